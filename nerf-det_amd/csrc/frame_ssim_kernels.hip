// Frame SSIM: the reference's second render metric (compute_ssim, mmdet3d/models/model_utils/save_rendered_img.py:21-36 ->
// skimage.metrics.structural_similarity(multichannel=True) of scikit-image 0.18.1: 7 x 7 uniform window, sample covariance, K1 = 0.01,
// K2 = 0.03, data range 2, the window-valid interior) on the device, for byte frames (kind 0) and float renders (kind 1).
//
//   k_frame_ssim<KIND>  a workgroup of 256 threads owns SSIM_TH x SSIM_TW windows of one frame.  It stages the (TH + 6) x (TW + 6) pixel patch
//       of both frames and the patch's "has depth" flags once (tile halos are the only re-reads), makes the horizontal 7-sum of the flags
//       (the sixth box sum: a window counts iff its 49 flags add to 49), and then per channel: the horizontal 7-sums of x, y, xx, yy, xy
//       into LDS (bytes: exact int32, x | y packed 16 + 16; floats: float64, the 7 terms added left to right), a barrier, and per thread the
//       vertical 7-sum (top to bottom) and the window expression for its two windows.  Every window forms its sums freshly, so its value
//       does not depend on where its tile starts.  s = (A1 A2) / (B1 B2) in float64, one rounding per operation (the file is compiled
//       with -ffp-contract=off), q = llrint(s * 2^40).  q (int64, may be negative) and the number of counting windows are reduced over
//       the wave with shuffles on both 32-bit halves, over the waves through LDS, and leave by one 64-bit vector atomic add per workgroup
//       and output word: integers, so the same bytes for any tile shape, launch geometry and order.  The sums are zeroed by a memset node
//       in front of the launch.
#include "ndet_common.hpp"

#define SSIM_TH 16
#define SSIM_TW 32
#define SSIM_WIN 7
#define SSIM_PH (SSIM_TH + SSIM_WIN - 1)       // patch rows
#define SSIM_PW (SSIM_TW + SSIM_WIN - 1)       // patch pixels per row
#define SSIM_ROWS_PER_THREAD (SSIM_TH * SSIM_TW / 256)

// (0.01 * 2 * 255)^2 * 49^2 and (0.03 * 2 * 255)^2 * 49 * 48, (0.01 * 2)^2 * 49^2 and (0.03 * 2)^2 * 49 * 48 as float64 evaluates them left
// to right (tests/frame_ssim_ref.py forms them the same way)
#define SSIM_C1_U8 0x1.e7e4051eb8520p+15
#define SSIM_C2_U8 0x1.0cd675c28f5c2p+19
#define SSIM_C1_F32 0x1.ebb98c7e28241p-1
#define SSIM_C2_F32 0x1.0ef34d6a161e5p+3

template <int KIND>
struct SsimKind;
template <>
struct SsimKind<0> {
    using In = uint8_t;
    using Sum = int;            // word 0: sum x | sum y << 16 (7 * 255 and 49 * 255 fit 16 bits), words 1..3: sums of xx, yy, xy
    static constexpr int kSums = 4;
};
template <>
struct SsimKind<1> {
    using In = float;
    using Sum = double;         // sums of x, y, xx, yy, xy
    static constexpr int kSums = 5;
};

// the window expression on the exact integer sums of 49 bytes.  Every int below fits: sx, sy <= 12495, so sx * sy, sx * sx <= 1.57e8 and
// their doubles and sums <= 3.13e8; 49 * sxy <= 49^2 * 255^2 = 1.57e8 and |49 * sxy - sx * sy| <= 1.57e8.  Integer reassociation keeps a value
// that fits, so no regrouping by the compiler can change these.
__device__ __forceinline__ long long ssim_q_u8(int sx, int sy, int sxx, int syy, int sxy) {
    const int pxy = sx * sy, pxx = sx * sx, pyy = sy * sy;
    const double a1 = (double)(2 * pxy) + SSIM_C1_U8;
    const double a2 = (double)(2 * (49 * sxy - pxy)) + SSIM_C2_U8;
    const double b1 = (double)(pxx + pyy) + SSIM_C1_U8;
    const double b2 = (double)((49 * sxx - pxx) + (49 * syy - pyy)) + SSIM_C2_U8;
    const double s = (a1 * a2) / (b1 * b2);
    return llrint(s * 0x1p40);
}

__device__ __forceinline__ long long ssim_q_f32(double sx, double sy, double sxx, double syy, double sxy) {
    const double pxy = sx * sy;
    const double a1 = 2.0 * pxy + SSIM_C1_F32;
    const double a2 = 2.0 * (49.0 * sxy - pxy) + SSIM_C2_F32;
    const double b1 = (sx * sx + sy * sy) + SSIM_C1_F32;
    const double b2 = ((49.0 * sxx - sx * sx) + (49.0 * syy - sy * sy)) + SSIM_C2_F32;
    const double s = (a1 * a2) / (b1 * b2);
    return llrint(s * 0x1p40);
}

template <int KIND>
__global__ __launch_bounds__(256) void k_frame_ssim(const typename SsimKind<KIND>::In* __restrict__ a, const typename SsimKind<KIND>::In* __restrict__ b,
                                                    const uint16_t* __restrict__ da /* may be null */, int h, int w, int tiles_x, int tiles_per_frame,
                                                    unsigned long long* __restrict__ out /* (n,4) */) {
    using In = typename SsimKind<KIND>::In;
    using Sum = typename SsimKind<KIND>::Sum;
    constexpr int kSums = SsimKind<KIND>::kSums;
    constexpr int kRow = SSIM_PW * 3;                                  // patch elements per row
    __shared__ In s_a[SSIM_PH][kRow], s_b[SSIM_PH][kRow];
    __shared__ uint8_t s_valid[SSIM_PH][SSIM_PW], s_hcnt[SSIM_PH][SSIM_TW];
    __shared__ Sum s_h[kSums][SSIM_PH][SSIM_TW];
    __shared__ unsigned long long s_part[256 / NDET_WAVE][4];

    const int tid = threadIdx.x;
    const int f = blockIdx.x / tiles_per_frame;
    const int t = blockIdx.x - f * tiles_per_frame;
    const int ty0 = (t / tiles_x) * SSIM_TH, tx0 = (t % tiles_x) * SSIM_TW;
    const int64_t frame = (int64_t)f * h * w;                          // pixels in front of this frame: n * h * w * 3 < 2^31

    // ---- stage the patch: every element once, zero beyond the frame
    const int row_elems = min(kRow, (w - tx0) * 3);
    for (int i = tid; i < SSIM_PH * kRow; i += 256) {
        const int r = i / kRow, e = i - r * kRow;
        const int y = ty0 + r;
        In va = (In)0, vb = (In)0;
        if (y < h && e < row_elems) {
            const int64_t at = (frame + (int64_t)y * w + tx0) * 3 + e;
            va = a[at];
            vb = b[at];
        }
        s_a[r][e] = va;
        s_b[r][e] = vb;
    }
    for (int i = tid; i < SSIM_PH * SSIM_PW; i += 256) {
        const int r = i / SSIM_PW, c = i - r * SSIM_PW;
        const int y = ty0 + r, x = tx0 + c;
        uint8_t v = 0;
        if (y < h && x < w) v = (da == nullptr || da[frame + (int64_t)y * w + x] != 0) ? 1 : 0;
        s_valid[r][c] = v;
    }
    __syncthreads();
    for (int i = tid; i < SSIM_PH * SSIM_TW; i += 256) {
        const int r = i / SSIM_TW, c = i - r * SSIM_TW;
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < SSIM_WIN; ++k) cnt += s_valid[r][c + k];
        s_hcnt[r][c] = (uint8_t)cnt;
    }
    __syncthreads();

    // this thread's windows: column wx, rows wy0 .. wy0 + SSIM_ROWS_PER_THREAD - 1 of the tile
    const int wx = tid % SSIM_TW, wy0 = (tid / SSIM_TW) * SSIM_ROWS_PER_THREAD;
    bool counts[SSIM_ROWS_PER_THREAD];
    int n_w = 0;
#pragma unroll
    for (int j = 0; j < SSIM_ROWS_PER_THREAD; ++j) {
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < SSIM_WIN; ++k) cnt += s_hcnt[wy0 + j + k][wx];
        counts[j] = cnt == SSIM_WIN * SSIM_WIN;                        // pixels beyond the frame carry flag 0: such a window never counts
        n_w += counts[j] ? 1 : 0;
    }

    long long acc[3] = {0, 0, 0};
    for (int c = 0; c < 3; ++c) {
        // ---- horizontal 7-sums of channel c, left to right
        for (int i = tid; i < SSIM_PH * SSIM_TW; i += 256) {
            const int r = i / SSIM_TW, x = i - r * SSIM_TW;
            if constexpr (KIND == 0) {
                int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
                for (int k = 0; k < SSIM_WIN; ++k) {
                    const int va = s_a[r][(x + k) * 3 + c], vb = s_b[r][(x + k) * 3 + c];
                    sx += va;
                    sy += vb;
                    sxx += va * va;
                    syy += vb * vb;
                    sxy += va * vb;
                }
                s_h[0][r][x] = sx | (sy << 16);
                s_h[1][r][x] = sxx;
                s_h[2][r][x] = syy;
                s_h[3][r][x] = sxy;
            } else {
                double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;     // 0.0 + v is v: the first term is taken as it is
#pragma unroll
                for (int k = 0; k < SSIM_WIN; ++k) {
                    const double va = (double)s_a[r][(x + k) * 3 + c], vb = (double)s_b[r][(x + k) * 3 + c];
                    sx += va;
                    sy += vb;
                    sxx += va * va;                                    // exact: a product of two float32
                    syy += vb * vb;
                    sxy += va * vb;
                }
                s_h[0][r][x] = sx;
                s_h[1][r][x] = sy;
                s_h[2][r][x] = sxx;
                s_h[3][r][x] = syy;
                s_h[4][r][x] = sxy;
            }
        }
        __syncthreads();
        // ---- vertical 7-sums, top to bottom, and the window expression
#pragma unroll
        for (int j = 0; j < SSIM_ROWS_PER_THREAD; ++j) {
            Sum v[kSums];
#pragma unroll
            for (int m = 0; m < kSums; ++m) {
                Sum sum = (Sum)0;
#pragma unroll
                for (int k = 0; k < SSIM_WIN; ++k) sum += s_h[m][wy0 + j + k][wx];
                v[m] = sum;
            }
            if (counts[j]) {
                if constexpr (KIND == 0) acc[c] += ssim_q_u8(v[0] & 0xffff, (int)((unsigned)v[0] >> 16), v[1], v[2], v[3]);
                else acc[c] += ssim_q_f32(v[0], v[1], v[2], v[3], v[4]);
            }
        }
        __syncthreads();
    }

    // ---- the workgroup's four sums: wave shuffles on both halves, the waves through LDS, one atomic add per word
    unsigned long long v[4] = {(unsigned long long)acc[0], (unsigned long long)acc[1], (unsigned long long)acc[2], (unsigned long long)n_w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int o = NDET_WAVE / 2; o > 0; o >>= 1) {
            const unsigned lo = __shfl_xor((unsigned)v[k], o), hi = __shfl_xor((unsigned)(v[k] >> 32), o);
            v[k] += ((unsigned long long)hi << 32) | lo;
        }
    const int lane = tid & (NDET_WAVE - 1), wave = tid / NDET_WAVE;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) s_part[wave][k] = v[k];
    __syncthreads();
    if (tid < 4) {
        unsigned long long sum = 0ull;
#pragma unroll
        for (int wv = 0; wv < 256 / NDET_WAVE; ++wv) sum += s_part[wv][tid];
        if (sum) atomicAdd(out + (int64_t)f * 4 + tid, sum);
    }
}

extern "C" int ndet_frame_ssim(const void* a, const void* b, const uint16_t* depth_a, int kind, int n, int h, int w, int64_t* out, void* stream) {
    const char* fn = "ndet_frame_ssim";
    NDET_REQUIRE(a && b && out, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(n >= 1 && h >= SSIM_WIN && w >= SSIM_WIN, NDET_E_INVALID, "%s: n = %d must be positive and h, w = %d, %d at least %d", fn, n, h, w,
                 SSIM_WIN);
    NDET_REQUIRE(kind == 0 || kind == 1, NDET_E_INVALID, "%s: kind %d is neither 0 (uint8) nor 1 (float32)", fn, kind);
    const int64_t windows = (int64_t)(h - SSIM_WIN + 1) * (w - SSIM_WIN + 1);
    NDET_REQUIRE(windows < ((int64_t)1 << 22), NDET_E_UNSUPPORTED, "%s: %lld windows a frame: 2^22 or more", fn, (long long)windows);
    NDET_REQUIRE((int64_t)n * h * w * 3 < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: %d frames of %d x %d pixels hold 2^31 elements or more", fn, n,
                 h, w);
    NDET_REQUIRE(((uintptr_t)depth_a & 1) == 0 && ((uintptr_t)out & 7) == 0, NDET_E_UNSUPPORTED,
                 "%s: depth_a must be 2-byte aligned, out 8-byte aligned", fn);
    NDET_REQUIRE(kind == 0 || (((uintptr_t)a | (uintptr_t)b) & 3) == 0, NDET_E_UNSUPPORTED, "%s: float32 frames must be 4-byte aligned", fn);
    const hipError_t e = hipMemsetAsync(out, 0, (size_t)n * 4 * sizeof(int64_t), (hipStream_t)stream);
    NDET_REQUIRE(e == hipSuccess, NDET_E_LAUNCH, "%s: cannot clear the sums: %s", fn, hipGetErrorString(e));
    const int tiles_x = (w - SSIM_WIN + 1 + SSIM_TW - 1) / SSIM_TW, tiles_y = (h - SSIM_WIN + 1 + SSIM_TH - 1) / SSIM_TH;
    const int tpf = tiles_x * tiles_y;                                 // n * tpf < n * h * w < 2^31
    const dim3 grid((unsigned)((int64_t)n * tpf));
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(out);
    if (kind == 0)
        hipLaunchKernelGGL(k_frame_ssim<0>, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const uint8_t*>(a), static_cast<const uint8_t*>(b),
                           depth_a, h, w, tiles_x, tpf, sums);
    else
        hipLaunchKernelGGL(k_frame_ssim<1>, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const float*>(a), static_cast<const float*>(b),
                           depth_a, h, w, tiles_x, tpf, sums);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}
