// The per-pixel body of the capture-resolution input contract (Resize(keep_ratio) -> Normalize -> Pad), shared by its two source formats:
// uint8 BGR frames (frame_kernels.hip) and NV12 surfaces (nv12_frames_kernels.hip).  One copy of the pad branch, of cv2.INTER_LINEAR's
// 2^11 fixed-point blend and of k_normalize_views' float32 arithmetic; what differs is how a tap's BGR triple is fetched:
//
//   struct Source {
//       __device__ const uint8_t* frame(int id) const;                                  // 64-bit frame offset
//       __device__ void tap(const uint8_t* frame, int y, int x, int bgr[3]) const;      // 32-bit offset inside the frame
//   };
#pragma once
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

struct FrameNorm {
    float mean[3], inv[3], sd[3];   // RGB
};

// One thread per pixel of the padded (n_sel, H, W) outputs; the caller's grid covers n_sel * H * W threads of 256 a workgroup.
template <class Source>
__device__ __forceinline__ void resize_normalize_pixel(const Source& source, const int* __restrict__ ids, int n_sel, int Hs, int Ws, int Hr, int Wr, int H,
                                                       int W, double sy, double sx, const FrameNorm& nm, float* __restrict__ img,
                                                       float* __restrict__ denorm, uint8_t* __restrict__ resized) {
    const int64_t hw = (int64_t)H * W;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_sel * hw) return;
    const int v = (int)(i / hw);
    const int64_t px = i - v * hw;
    const int y = (int)(px / W), x = (int)(px - (int64_t)y * W);
    float* im = img + (int64_t)v * 3 * hw + px;
    float* dn = denorm + (int64_t)v * 3 * hw + px;
    if (y >= Hr || x >= Wr) {   // Pad(pad_val=0) of the normalised image
#pragma unroll
        for (int c = 0; c < 3; ++c) {   // c indexes RGB
            im[c * hw] = 0.0f;
            dn[(2 - c) * hw] = (float)(unsigned char)(int)nm.mean[c] / 255.0f;   // 0 * std + mean, .astype(np.uint8)
        }
        if (resized) {
            uint8_t* r = resized + i * 3;
            r[0] = 0; r[1] = 0; r[2] = 0;
        }
        return;
    }
    const FrameTap ty = frame_tap(y, sy, Hs), tx = frame_tap(x, sx, Ws);
    const uint8_t* src = source.frame(ids ? ids[v] : v);
    int p00[3], p01[3], p10[3], p11[3];
    source.tap(src, ty.s0, tx.s0, p00);
    source.tap(src, ty.s0, tx.s1, p01);
    source.tap(src, ty.s1, tx.s0, p10);
    source.tap(src, ty.s1, tx.s1, p11);
    int bgr[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const int h0 = p00[b] * tx.a0 + p01[b] * tx.a1;   // horizontal pass, scaled by 2^11
        const int h1 = p10[b] * tx.a0 + p11[b] * tx.a1;
        int o = (((ty.a0 * (h0 >> 4)) >> 16) + ((ty.a1 * (h1 >> 4)) >> 16) + 2) >> 2;
        bgr[b] = o > 255 ? 255 : o;                        // np.clip; no term is negative
    }
    if (resized) {
        uint8_t* r = resized + i * 3;
        r[0] = (uint8_t)bgr[0]; r[1] = (uint8_t)bgr[1]; r[2] = (uint8_t)bgr[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {   // c indexes RGB; the arithmetic of k_normalize_views
        const float xn = ((float)bgr[2 - c] - nm.mean[c]) * nm.inv[c];
        im[c * hw] = xn;
        const float back = xn * nm.sd[c] + nm.mean[c];                // imdenormalize
        const float q = (float)(unsigned char)(int)back;              // .astype(np.uint8): truncation
        dn[(2 - c) * hw] = q / 255.0f;                                // BGR planes
    }
}

// What both entry points refuse of the arguments they share, in two steps around the source's own size check: the normalisation (which
// fills the kernel's FrameNorm) and the pad, then the output planes and the grid.  NDET_OK, or the refusal's code with the message set.
static inline int frame_norm_checks(const char* fn, int Hr, int Wr, int H, int W, const double* mean_rgb, const double* std_rgb, FrameNorm* nm) {
    for (int c = 0; c < 3; ++c) {
        NDET_REQUIRE(std_rgb[c] > 0.0, NDET_E_INVALID, "%s: std must be positive", fn);
        nm->inv[c] = (float)(1.0 / std_rgb[c]);   // mmcv: stdinv = 1 / np.float64(std), applied to the float32 image
        nm->mean[c] = (float)mean_rgb[c];
        nm->sd[c] = (float)std_rgb[c];
    }
    NDET_REQUIRE(Hr <= H && Wr <= W, NDET_E_INVALID, "%s: the resized frame %d x %d does not fit the pad %d x %d", fn, Hr, Wr, H, W);
    return NDET_OK;
}

static inline int frame_grid_checks(const char* fn, int n_sel, int H, int W, int64_t* blocks) {
    NDET_REQUIRE((int64_t)H * W * 3 < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: a view's planes %d x %d x 3 hold 2^31 elements or more", fn, H, W);
    *blocks = ((int64_t)n_sel * H * W + 255) / 256;
    NDET_REQUIRE(*blocks < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: %d views of %d x %d need 2^31 workgroups or more", fn, n_sel, H, W);
    return NDET_OK;
}
