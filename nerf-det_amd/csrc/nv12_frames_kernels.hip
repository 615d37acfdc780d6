// NV12 surfaces in and out: what a hardware video decoder leaves in device memory and what a hardware encoder takes.  A surface batch is
// uint8 (n, rows, pitch): the Y plane in rows [0, Hs), the interleaved U,V plane (U first) in rows [uv_row, uv_row + Hs / 2), columns
// [0, Ws) of each row used; tight is pitch = Ws, uv_row = Hs, rows = Hs * 3 / 2.  Hs and Ws are even.
//
//   The colour definition is datasets.nv12_to_bgr / datasets.bgr_to_nv12 (BT.601 limited range in 20-bit fixed point, the constants of
//   OpenCV's COLOR_YUV2BGR_NV12 / COLOR_BGR2YUV family; nearest chroma on ingest, the rounded 2 x 2 mean on egress):
//       Y' = max(0, Y - 16) * 1220542, u = U - 128, v = V - 128, h = 1 << 19
//       R = (Y' + h + 1673527 v) >> 20, G = (Y' + h - 852492 v - 409993 u) >> 20, B = (Y' + h + 2116026 u) >> 20, clipped to [0, 255]
//   with an arithmetic shift; |Y' + h + 2116026 u| < 5.7e8 fits int32.
//
//   k_resize_normalize_views_nv12   k_resize_normalize_views (frame_kernels.hip) reading surfaces: frame_resize.hpp's per-pixel body with a
//       tap that takes Y at (y, x) and the UV pair at (y >> 1, x >> 1) -- one 16-bit load, hence the even pitch and base -- and converts its
//       own pixel before the blend.  The outputs are what ndet_resize_normalize_views writes for nv12_to_bgr of each surface, bit for bit.
//   k_nv12_to_bgr                   surfaces -> (n_sel, Hs, Ws, 3) BGR at full size; one thread per 2 x 2 block, so each UV pair is read once.
//   k_bgr_to_nv12                   (n, H, W, 3) BGR of any size -> tight surfaces of He x We (H, W rounded up to even, the last row / column
//                                   replicated); one thread per 2 x 2 block writes four Y bytes and one UV pair; every output byte is written.
#include "ndet_common.hpp"
#include "frame_resize.hpp"

__device__ __forceinline__ void nv12_pixel_bgr(int Y, int U, int V, int bgr[3]) {
    const int yy = (Y > 16 ? Y - 16 : 0) * 1220542 + (1 << 19);
    const int u = U - 128, v = V - 128;
    const int r = (yy + 1673527 * v) >> 20;   // arithmetic shift: floor
    const int g = (yy - 852492 * v - 409993 * u) >> 20;
    const int b = (yy + 2116026 * u) >> 20;
    bgr[0] = b < 0 ? 0 : (b > 255 ? 255 : b);
    bgr[1] = g < 0 ? 0 : (g > 255 ? 255 : g);
    bgr[2] = r < 0 ? 0 : (r > 255 ? 255 : r);
}

struct Nv12Surfaces {
    const uint8_t* surfaces;
    int pitch, uv_row, rows;
    __device__ __forceinline__ const uint8_t* frame(int id) const { return surfaces + (int64_t)id * rows * pitch; }   // rows * pitch < 2^31
    __device__ __forceinline__ void tap(const uint8_t* src, int y, int x, int bgr[3]) const {
        const int Y = (int)src[y * pitch + x];
        const unsigned uv = *(const uint16_t*)(src + (uv_row + (y >> 1)) * pitch + (x >> 1) * 2);   // even pitch and base: aligned
        nv12_pixel_bgr(Y, (int)(uv & 0xffu), (int)(uv >> 8), bgr);
    }
};

__global__ __launch_bounds__(256) void k_resize_normalize_views_nv12(const uint8_t* __restrict__ surfaces, const int* __restrict__ ids, int n_sel, int Hs,
                                                                     int Ws, int pitch, int uv_row, int rows, int Hr, int Wr, int H, int W, double sy,
                                                                     double sx, float m0, float m1, float m2, float i0, float i1, float i2, float s0,
                                                                     float s1, float s2, float* __restrict__ img, float* __restrict__ denorm,
                                                                     uint8_t* __restrict__ resized) {
    const FrameNorm nm = {{m0, m1, m2}, {i0, i1, i2}, {s0, s1, s2}};
    resize_normalize_pixel(Nv12Surfaces{surfaces, pitch, uv_row, rows}, ids, n_sel, Hs, Ws, Hr, Wr, H, W, sy, sx, nm, img, denorm, resized);
}

__global__ __launch_bounds__(256) void k_nv12_to_bgr(const uint8_t* __restrict__ surfaces, const int* __restrict__ ids, int n_sel, int Hs, int Ws, int pitch,
                                                     int uv_row, int rows, uint8_t* __restrict__ out) {
    const int bw = Ws >> 1;
    const int64_t per = (int64_t)(Hs >> 1) * bw;   // 2 x 2 blocks of a frame
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_sel * per) return;
    const int v = (int)(i / per);
    const int blk = (int)(i - v * per);
    const int by = blk / bw, bx = blk - by * bw;
    const uint8_t* src = surfaces + (int64_t)(ids ? ids[v] : v) * rows * pitch;
    const unsigned uv = *(const uint16_t*)(src + (uv_row + by) * pitch + bx * 2);
    const int U = (int)(uv & 0xffu), V = (int)(uv >> 8);
    uint8_t* dst = out + (int64_t)v * Hs * Ws * 3;   // one frame holds fewer than 2^31 bytes
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int y = 2 * by + dy;
        const unsigned yy = *(const uint16_t*)(src + y * pitch + 2 * bx);   // the block's two Y bytes of this row
        uint8_t* o = dst + (y * Ws + 2 * bx) * 3;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            int bgr[3];
            nv12_pixel_bgr((int)((yy >> (8 * dx)) & 0xffu), U, V, bgr);
            o[3 * dx + 0] = (uint8_t)bgr[0]; o[3 * dx + 1] = (uint8_t)bgr[1]; o[3 * dx + 2] = (uint8_t)bgr[2];
        }
    }
}

__global__ __launch_bounds__(256) void k_bgr_to_nv12(const uint8_t* __restrict__ frames, int n, int H, int W, int He, int We, uint8_t* __restrict__ surfaces) {
    const int bw = We >> 1;
    const int64_t per = (int64_t)(He >> 1) * bw;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * per) return;
    const int v = (int)(i / per);
    const int blk = (int)(i - v * per);
    const int by = blk / bw, bx = blk - by * bw;
    const uint8_t* src = frames + (int64_t)v * H * W * 3;
    uint8_t* dst = surfaces + (int64_t)v * (He / 2 * 3) * We;   // He * 3 / 2 rows of We bytes
    int sum[3] = {0, 0, 0};
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int y = 2 * by + dy, ys = y < H ? y : H - 1;      // the last row, replicated
        uint8_t yb[2];
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int x = 2 * bx + dx, xs = x < W ? x : W - 1;  // the last column, replicated
            const uint8_t* p = src + (ys * W + xs) * 3;
            const int B = (int)p[0], G = (int)p[1], R = (int)p[2];
            sum[0] += B; sum[1] += G; sum[2] += R;
            yb[dx] = (uint8_t)((269484 * R + 528482 * G + 102760 * B + (16 << 20) + (1 << 19)) >> 20);   // 16 .. 235: no clip needed
        }
        uint8_t* o = dst + y * We + 2 * bx;
        o[0] = yb[0]; o[1] = yb[1];
    }
    const int B = (sum[0] + 2) >> 2, G = (sum[1] + 2) >> 2, R = (sum[2] + 2) >> 2;   // the rounded 2 x 2 mean per channel
    int U = (-155188 * R - 305135 * G + 460324 * B + (128 << 20) + (1 << 19)) >> 20;
    int V = (460324 * R - 385875 * G - 74448 * B + (128 << 20) + (1 << 19)) >> 20;
    U = U < 0 ? 0 : (U > 255 ? 255 : U);
    V = V < 0 ? 0 : (V > 255 ? 255 : V);
    uint8_t* o = dst + (He + by) * We + 2 * bx;
    o[0] = (uint8_t)U; o[1] = (uint8_t)V;
}

// What both ingest entry points refuse of a surface batch's description.
static int nv12_surface_checks(const char* fn, const void* surfaces, int Hs, int Ws, int pitch, int uv_row, int rows) {
    NDET_REQUIRE(Hs % 2 == 0 && Ws % 2 == 0, NDET_E_INVALID, "%s: an NV12 surface of %d x %d must have even sizes", fn, Hs, Ws);
    NDET_REQUIRE(pitch >= Ws, NDET_E_INVALID, "%s: pitch %d is below the width %d", fn, pitch, Ws);
    NDET_REQUIRE(uv_row >= Hs, NDET_E_INVALID, "%s: uv_row %d lies inside the Y plane of %d rows", fn, uv_row, Hs);
    NDET_REQUIRE((int64_t)rows >= (int64_t)uv_row + Hs / 2, NDET_E_INVALID, "%s: %d rows do not hold a UV plane of %d rows at row %d", fn, rows, Hs / 2, uv_row);
    NDET_REQUIRE((int64_t)rows * pitch < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: a surface of %d rows x %d bytes holds 2^31 bytes or more", fn, rows, pitch);
    NDET_REQUIRE(pitch % 2 == 0 && ((uintptr_t)surfaces & 1) == 0, NDET_E_UNSUPPORTED,
                 "%s: an odd pitch (%d) or base address is not supported: the UV pair is one 16-bit load", fn, pitch);
    return NDET_OK;
}

extern "C" int ndet_resize_normalize_views_nv12(const uint8_t* surfaces, const int* ids, int n_sel, int Hs, int Ws, int pitch, int uv_row, int rows, int Hr,
                                                int Wr, int H, int W, const double* mean_rgb, const double* std_rgb, float* img, float* denorm,
                                                uint8_t* resized_bgr, void* stream) {
    const char* fn = "ndet_resize_normalize_views_nv12";
    NDET_REQUIRE(surfaces && mean_rgb && std_rgb && img && denorm, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(n_sel > 0 && Hs > 0 && Ws > 0 && pitch > 0 && uv_row > 0 && rows > 0 && Hr > 0 && Wr > 0 && H > 0 && W > 0, NDET_E_INVALID,
                 "%s: sizes must be positive", fn);
    FrameNorm nm;
    NDET_TRY(frame_norm_checks(fn, Hr, Wr, H, W, mean_rgb, std_rgb, &nm));
    NDET_TRY(nv12_surface_checks(fn, surfaces, Hs, Ws, pitch, uv_row, rows));
    int64_t blocks;
    NDET_TRY(frame_grid_checks(fn, n_sel, H, W, &blocks));
    hipLaunchKernelGGL(k_resize_normalize_views_nv12, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, surfaces, ids, n_sel, Hs, Ws, pitch, uv_row,
                       rows, Hr, Wr, H, W, (double)Hs / (double)Hr, (double)Ws / (double)Wr, nm.mean[0], nm.mean[1], nm.mean[2], nm.inv[0], nm.inv[1], nm.inv[2], nm.sd[0],
                       nm.sd[1], nm.sd[2], img, denorm, resized_bgr);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_nv12_to_bgr(const uint8_t* surfaces, const int* ids, int n_sel, int Hs, int Ws, int pitch, int uv_row, int rows, uint8_t* frames_bgr,
                                void* stream) {
    const char* fn = "ndet_nv12_to_bgr";
    NDET_REQUIRE(surfaces && frames_bgr, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(n_sel > 0 && Hs > 0 && Ws > 0 && pitch > 0 && uv_row > 0 && rows > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    NDET_TRY(nv12_surface_checks(fn, surfaces, Hs, Ws, pitch, uv_row, rows));
    NDET_REQUIRE((int64_t)Hs * Ws * 3 < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: a frame of %d x %d x 3 holds 2^31 elements or more", fn, Hs, Ws);
    const int64_t blocks = ((int64_t)n_sel * (Hs / 2) * (Ws / 2) + 255) / 256;
    NDET_REQUIRE(blocks < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: %d frames of %d x %d need 2^31 workgroups or more", fn, n_sel, Hs, Ws);
    hipLaunchKernelGGL(k_nv12_to_bgr, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, surfaces, ids, n_sel, Hs, Ws, pitch, uv_row, rows, frames_bgr);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_bgr_to_nv12(const uint8_t* frames_bgr, int n, int H, int W, uint8_t* surfaces, void* stream) {
    const char* fn = "ndet_bgr_to_nv12";
    NDET_REQUIRE(frames_bgr && surfaces, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(n > 0 && H > 0 && W > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    NDET_REQUIRE((int64_t)H * W * 3 < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: a frame of %d x %d x 3 holds 2^31 elements or more", fn, H, W);
    const int He = H + (H & 1), We = W + (W & 1);   // below 2^31: H * W * 3 is
    const int64_t blocks = ((int64_t)n * (He / 2) * (We / 2) + 255) / 256;
    NDET_REQUIRE(blocks < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: %d frames of %d x %d need 2^31 workgroups or more", fn, n, H, W);
    hipLaunchKernelGGL(k_bgr_to_nv12, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames_bgr, n, H, W, He, We, surfaces);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}
