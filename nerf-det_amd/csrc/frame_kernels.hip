// Input contract from frames at CAPTURE resolution: Resize(keep_ratio) -> Normalize -> Pad of the nerfdet configs in one launch, for
// uint8 BGR frames resident on the device (what a decode engine leaves there).
//
//   k_resize_normalize_views   per selected frame and pixel of the padded H x W image:
//       content [0,Hr) x [0,Wr): the byte of datasets.imresize_linear(frame, (Wr, Hr)) -- cv2.INTER_LINEAR's two taps per axis at half-pixel
//                                centres, 11-bit fixed-point weights, two-stage rounding (resize.cpp) -- then k_normalize_views' float32
//                                arithmetic on that byte: img = mmcv.imnormalize(to_rgb=True), denorm = the truncating uint8 round trip / 255;
//       pad, the rest:           img = 0 (Pad comes after Normalize), denorm = trunc(mean) / 255 (what the round trip makes of a zero),
//                                resized byte 0.
//   The taps are computed per thread: position float32(float64((d + 0.5) * (src / dst) - 0.5)), floor, clamp at both borders (only an
//   upscale reaches them), weights rint(f * 2048) and rint((1 - f) * 2048).  Hr == Hs && Wr == Ws gives position d and weights
//   (2048, 0) on both axes, and ((2048 * (2048 * p >> 4) >> 16) + 2) >> 2 == p: the copy the host function makes.  Every intermediate
//   fits int32: 2049 * ((255 * 2049) >> 4) < 2^26.
#include "ndet_common.hpp"
#include "frame_tap.hpp"

struct FrameTap {
    int s0, s1;   // source index of the two taps
    int a0, a1;   // their weights, scaled by 2^11
};

__device__ __forceinline__ FrameTap frame_tap(int d, double scale /* n_src / n_dst */, int n_src) {
    const FramePos p = frame_pos(d, scale, n_src);
    FrameTap t;
    t.s0 = p.s0;
    t.s1 = p.s1;
    t.a1 = (int)rintf(p.f * 2048.0f);
    t.a0 = (int)rintf((1.0f - p.f) * 2048.0f);
    return t;
}

__global__ __launch_bounds__(256) void k_resize_normalize_views(const uint8_t* __restrict__ frames, const int* __restrict__ ids, int n_sel, int Hs, int Ws,
                                                                int Hr, int Wr, int H, int W, double sy, double sx, float m0, float m1, float m2,
                                                                float i0, float i1, float i2, float s0, float s1, float s2, float* __restrict__ img,
                                                                float* __restrict__ denorm, uint8_t* __restrict__ resized) {
    const int64_t hw = (int64_t)H * W;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_sel * hw) return;
    const int v = (int)(i / hw);
    const int64_t px = i - v * hw;
    const int y = (int)(px / W), x = (int)(px - (int64_t)y * W);
    const float mean[3] = {m0, m1, m2}, inv[3] = {i0, i1, i2}, sd[3] = {s0, s1, s2};
    float* im = img + (int64_t)v * 3 * hw + px;
    float* dn = denorm + (int64_t)v * 3 * hw + px;
    if (y >= Hr || x >= Wr) {   // Pad(pad_val=0) of the normalised image
#pragma unroll
        for (int c = 0; c < 3; ++c) {   // c indexes RGB
            im[c * hw] = 0.0f;
            dn[(2 - c) * hw] = (float)(unsigned char)(int)mean[c] / 255.0f;   // 0 * std + mean, .astype(np.uint8)
        }
        if (resized) {
            uint8_t* r = resized + i * 3;
            r[0] = 0; r[1] = 0; r[2] = 0;
        }
        return;
    }
    const FrameTap ty = frame_tap(y, sy, Hs), tx = frame_tap(x, sx, Ws);
    const uint8_t* src = frames + (int64_t)(ids ? ids[v] : v) * Hs * Ws * 3;   // one frame holds fewer than 2^31 bytes
    const uint8_t* p00 = src + (ty.s0 * Ws + tx.s0) * 3;
    const uint8_t* p01 = src + (ty.s0 * Ws + tx.s1) * 3;
    const uint8_t* p10 = src + (ty.s1 * Ws + tx.s0) * 3;
    const uint8_t* p11 = src + (ty.s1 * Ws + tx.s1) * 3;
    int bgr[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const int h0 = (int)p00[b] * tx.a0 + (int)p01[b] * tx.a1;   // horizontal pass, scaled by 2^11
        const int h1 = (int)p10[b] * tx.a0 + (int)p11[b] * tx.a1;
        int o = (((ty.a0 * (h0 >> 4)) >> 16) + ((ty.a1 * (h1 >> 4)) >> 16) + 2) >> 2;
        bgr[b] = o > 255 ? 255 : o;                                 // np.clip; no term is negative
    }
    if (resized) {
        uint8_t* r = resized + i * 3;
        r[0] = (uint8_t)bgr[0]; r[1] = (uint8_t)bgr[1]; r[2] = (uint8_t)bgr[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {   // c indexes RGB; the arithmetic of k_normalize_views
        const float xn = ((float)bgr[2 - c] - mean[c]) * inv[c];
        im[c * hw] = xn;
        const float back = xn * sd[c] + mean[c];                      // imdenormalize
        const float q = (float)(unsigned char)(int)back;              // .astype(np.uint8): truncation
        dn[(2 - c) * hw] = q / 255.0f;                                // BGR planes
    }
}

extern "C" int ndet_resize_normalize_views(const uint8_t* frames_bgr, const int* ids, int n_sel, int Hs, int Ws, int Hr, int Wr, int H, int W,
                                           const double* mean_rgb, const double* std_rgb, float* img, float* denorm, uint8_t* resized_bgr,
                                           void* stream) {
    const char* fn = "ndet_resize_normalize_views";
    NDET_REQUIRE(frames_bgr && mean_rgb && std_rgb && img && denorm, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(n_sel > 0 && Hs > 0 && Ws > 0 && Hr > 0 && Wr > 0 && H > 0 && W > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    float inv[3], mean[3], sd[3];
    for (int c = 0; c < 3; ++c) {
        NDET_REQUIRE(std_rgb[c] > 0.0, NDET_E_INVALID, "%s: std must be positive", fn);
        inv[c] = (float)(1.0 / std_rgb[c]);   // mmcv: stdinv = 1 / np.float64(std), applied to the float32 image
        mean[c] = (float)mean_rgb[c];
        sd[c] = (float)std_rgb[c];
    }
    NDET_REQUIRE(Hr <= H && Wr <= W, NDET_E_INVALID, "%s: the resized frame %d x %d does not fit the pad %d x %d", fn, Hr, Wr, H, W);
    NDET_REQUIRE((int64_t)Hs * Ws * 3 < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: a frame of %d x %d x 3 holds 2^31 elements or more", fn, Hs, Ws);
    NDET_REQUIRE((int64_t)H * W * 3 < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: a view's planes %d x %d x 3 hold 2^31 elements or more", fn, H, W);
    const int64_t blocks = ((int64_t)n_sel * H * W + 255) / 256;
    NDET_REQUIRE(blocks < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: %d views of %d x %d need 2^31 workgroups or more", fn, n_sel, H, W);
    hipLaunchKernelGGL(k_resize_normalize_views, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames_bgr, ids, n_sel, Hs, Ws, Hr, Wr, H, W,
                       (double)Hs / (double)Hr, (double)Ws / (double)Wr, mean[0], mean[1], mean[2], inv[0], inv[1], inv[2], sd[0], sd[1], sd[2], img,
                       denorm, resized_bgr);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}
