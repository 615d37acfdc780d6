// Input contract from frames at CAPTURE resolution: Resize(keep_ratio) -> Normalize -> Pad of the nerfdet configs in one launch, for
// uint8 BGR frames resident on the device.  (A hardware video decoder leaves NV12 surfaces: nv12_frames_kernels.hip takes those.)
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
//   The per-pixel body is frame_resize.hpp's resize_normalize_pixel, shared with the NV12 source; this file says how a BGR tap is fetched.
#include "ndet_common.hpp"
#include "frame_resize.hpp"

struct BgrFrames {
    const uint8_t* frames;
    int Hs, Ws;
    __device__ __forceinline__ const uint8_t* frame(int id) const { return frames + (int64_t)id * Hs * Ws * 3; }   // one frame holds fewer than 2^31 bytes
    __device__ __forceinline__ void tap(const uint8_t* src, int y, int x, int bgr[3]) const {
        const uint8_t* p = src + (y * Ws + x) * 3;
        bgr[0] = (int)p[0]; bgr[1] = (int)p[1]; bgr[2] = (int)p[2];
    }
};

__global__ __launch_bounds__(256) void k_resize_normalize_views(const uint8_t* __restrict__ frames, const int* __restrict__ ids, int n_sel, int Hs, int Ws,
                                                                int Hr, int Wr, int H, int W, double sy, double sx, float m0, float m1, float m2,
                                                                float i0, float i1, float i2, float s0, float s1, float s2, float* __restrict__ img,
                                                                float* __restrict__ denorm, uint8_t* __restrict__ resized) {
    const FrameNorm nm = {{m0, m1, m2}, {i0, i1, i2}, {s0, s1, s2}};
    resize_normalize_pixel(BgrFrames{frames, Hs, Ws}, ids, n_sel, Hs, Ws, Hr, Wr, H, W, sy, sx, nm, img, denorm, resized);
}

extern "C" int ndet_resize_normalize_views(const uint8_t* frames_bgr, const int* ids, int n_sel, int Hs, int Ws, int Hr, int Wr, int H, int W,
                                           const double* mean_rgb, const double* std_rgb, float* img, float* denorm, uint8_t* resized_bgr,
                                           void* stream) {
    const char* fn = "ndet_resize_normalize_views";
    NDET_REQUIRE(frames_bgr && mean_rgb && std_rgb && img && denorm, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(n_sel > 0 && Hs > 0 && Ws > 0 && Hr > 0 && Wr > 0 && H > 0 && W > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    FrameNorm nm;
    NDET_TRY(frame_norm_checks(fn, Hr, Wr, H, W, mean_rgb, std_rgb, &nm));
    NDET_REQUIRE((int64_t)Hs * Ws * 3 < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: a frame of %d x %d x 3 holds 2^31 elements or more", fn, Hs, Ws);
    int64_t blocks;
    NDET_TRY(frame_grid_checks(fn, n_sel, H, W, &blocks));
    hipLaunchKernelGGL(k_resize_normalize_views, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames_bgr, ids, n_sel, Hs, Ws, Hr, Wr, H, W,
                       (double)Hs / (double)Hr, (double)Ws / (double)Wr, nm.mean[0], nm.mean[1], nm.mean[2], nm.inv[0], nm.inv[1], nm.inv[2], nm.sd[0], nm.sd[1],
                       nm.sd[2], img, denorm, resized_bgr);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}
