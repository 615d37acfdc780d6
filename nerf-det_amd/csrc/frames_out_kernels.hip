// Frames out: the output side of a camera server -- a pose in, uint8 BGR and uint16 millimetre frames out, and a render compared with a
// held-out frame on the device (the reference writes its renders with np.uint8(img * 255) and scores them with compute_psnr:
// mmdet3d/models/model_utils/save_rendered_img.py:10-19,55,68).  Three memory-bound kernels, one element per thread, plain vector stores.
//
//   k_camera_rays   get_dtu_raydir (data_augment_utils.py:410-424, un-normalised) for the pixels px = x0 + j * stride, py = y0 + i * stride of
//       n cameras that share one pair of intrinsic rows: k_target_rays' directions (pipeline_kernels.hip) without its frame, both through
//       ndet_pixel_dir -- x = ((float)px + 0.5f - k[2]) / k[0], y likewise, d_j = fmaf(y, R[j][1], x * R[j][0]) + R[j][2] -- and the
//       camera centre repeated per ray.  No image bound: a pose may look anywhere.
//   k_pack_frames   float rgb in [0, 1] -> bytes, float metres -> uint16 millimetres, both round-half-up with saturation; NaN gives 0;
//       a ray whose mask is false gets depth 0, the sensor's hole.  Channel order is kept (the bank's images are BGR planes already).
//   k_frame_errors  per frame the four integer sums of a byte / millimetre comparison over the pixels where frame a has depth.  Every
//       term is an integer, so the wave reduction and the one 64-bit vector atomic add per workgroup and sum are exact and give the same
//       bytes in any order.  The sums are zeroed by a memset node in front of the launch.
#include "ndet_common.hpp"

__global__ __launch_bounds__(256) void k_camera_rays(const float* __restrict__ kn /* (2,3) */, const float* __restrict__ rot /* (n,3,3) */,
                                                     const float* __restrict__ lpos /* (n,3) */, int n_cams, int x0, int y0, int stride, int h, int w,
                                                     float* __restrict__ ray_o, float* __restrict__ ray_d) {
    const int64_t per = (int64_t)h * w;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cams * per) return;
    const int c = (int)(i / per);
    const int r = (int)(i - c * per);                 // one camera holds fewer than 2^31 rays
    const int row = r / w, col = r - row * w;
    const int px = x0 + col * stride, py = y0 + row * stride;
    float d[3];
    ndet_pixel_dir(kn, rot + (int64_t)c * 9, px, py, d);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        ray_d[i * 3 + j] = d[j];
        ray_o[i * 3 + j] = lpos[(int64_t)c * 3 + j];
    }
}

// v in units of the output: NaN and v < 0 give 0, v > hi gives hi, else trunc(v + 0.5f)
__device__ __forceinline__ int fo_quantise(float v, float hi) {
    if (!(v >= 0.0f)) return 0;
    if (v > hi) return (int)hi;
    return (int)(v + 0.5f);
}

__global__ __launch_bounds__(256) void k_pack_frames(const float* __restrict__ rgb, const float* __restrict__ depth, const uint8_t* __restrict__ mask,
                                                     int n, uint8_t* __restrict__ bgr_u8, uint16_t* __restrict__ depth_mm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) bgr_u8[(int64_t)i * 3 + c] = (uint8_t)fo_quantise(rgb[(int64_t)i * 3 + c] * 255.0f, 255.0f);
    const int mm = fo_quantise(depth[i] * 1000.0f, 65535.0f);
    depth_mm[i] = (uint16_t)((mask == nullptr || mask[i]) ? mm : 0);
}

__global__ __launch_bounds__(256) void k_frame_errors(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, const uint16_t* __restrict__ da,
                                                      const uint16_t* __restrict__ db, int px, int blocks_per_frame,
                                                      unsigned long long* __restrict__ out /* (n,4) */) {
    __shared__ unsigned s_part[256 / NDET_WAVE][4];
    const int f = blockIdx.x / blocks_per_frame;
    const int p = (blockIdx.x - f * blocks_per_frame) * 256 + threadIdx.x;
    unsigned v[4] = {0u, 0u, 0u, 0u};                 // sse, n_px, sad_mm, n_depth of this pixel: a workgroup's sums stay below 2^26
    if (p < px) {
        const int64_t at = (int64_t)f * px + p;
        const int za = da[at];
        if (za != 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int e = (int)a[at * 3 + c] - (int)b[at * 3 + c];
                v[0] += (unsigned)(e * e);
            }
            v[1] = 1u;
            const int zb = db ? db[at] : 0;
            if (zb != 0) {
                v[2] = (unsigned)(za > zb ? za - zb : zb - za);
                v[3] = 1u;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int o = NDET_WAVE / 2; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
    const int lane = threadIdx.x & (NDET_WAVE - 1), wave = threadIdx.x / NDET_WAVE;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) s_part[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned sum = 0u;
#pragma unroll
        for (int wv = 0; wv < 256 / NDET_WAVE; ++wv) sum += s_part[wv][threadIdx.x];
        if (sum) atomicAdd(out + (int64_t)f * 4 + threadIdx.x, (unsigned long long)sum);
    }
}

extern "C" int ndet_camera_rays(const float* intrinsic_rows, const float* camrotc2w, const float* cam_lightpos, int n_cams, int x0, int y0,
                                int stride, int h, int w, float* ray_o, float* ray_d, void* stream) {
    const char* fn = "ndet_camera_rays";
    NDET_REQUIRE(intrinsic_rows && camrotc2w && cam_lightpos && ray_o && ray_d, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(n_cams > 0 && h > 0 && w > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    NDET_REQUIRE(stride >= 1 && x0 >= 0 && y0 >= 0, NDET_E_INVALID, "%s: stride %d must be at least 1 and the offsets (%d, %d) non-negative", fn, stride,
                 x0, y0);
    NDET_REQUIRE((((uintptr_t)intrinsic_rows | (uintptr_t)camrotc2w | (uintptr_t)cam_lightpos | (uintptr_t)ray_o | (uintptr_t)ray_d) & 3) == 0,
                 NDET_E_UNSUPPORTED, "%s: pointers must be 4-byte aligned", fn);
    const int64_t two31 = (int64_t)1 << 31;
    NDET_REQUIRE(x0 + (int64_t)(w - 1) * stride < two31 && y0 + (int64_t)(h - 1) * stride < two31, NDET_E_UNSUPPORTED,
                 "%s: the last pixel lies at 2^31 or beyond", fn);
    NDET_REQUIRE((int64_t)h * w < two31 && (int64_t)n_cams * h * w * 3 < two31, NDET_E_UNSUPPORTED,
                 "%s: %d cameras of %d x %d rays hold 2^31 elements or more", fn, n_cams, h, w);
    const int64_t total = (int64_t)n_cams * h * w;
    hipLaunchKernelGGL(k_camera_rays, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, intrinsic_rows, camrotc2w, cam_lightpos,
                       n_cams, x0, y0, stride, h, w, ray_o, ray_d);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_pack_frames(const float* rgb, const float* depth, const uint8_t* mask, int64_t R, uint8_t* bgr_u8, uint16_t* depth_mm,
                                void* stream) {
    const char* fn = "ndet_pack_frames";
    NDET_REQUIRE(rgb && depth && bgr_u8 && depth_mm, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(R > 0, NDET_E_INVALID, "%s: R must be positive", fn);
    NDET_REQUIRE(R * 3 < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: R = %lld: 2^31 colour elements or more", fn, (long long)R);
    NDET_REQUIRE((((uintptr_t)rgb | (uintptr_t)depth) & 3) == 0 && ((uintptr_t)depth_mm & 1) == 0, NDET_E_UNSUPPORTED,
                 "%s: rgb and depth must be 4-byte aligned, depth_mm 2-byte aligned", fn);
    hipLaunchKernelGGL(k_pack_frames, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rgb, depth, mask, (int)R, bgr_u8, depth_mm);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_frame_errors(const uint8_t* a, const uint8_t* b, const uint16_t* da, const uint16_t* db, int n, int64_t px, int64_t* out,
                                 void* stream) {
    const char* fn = "ndet_frame_errors";
    NDET_REQUIRE(a && b && da && out, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(n > 0 && px > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    NDET_REQUIRE(px < ((int64_t)1 << 31) && (int64_t)n * px * 3 < ((int64_t)1 << 31), NDET_E_UNSUPPORTED,
                 "%s: %d frames of %lld pixels hold 2^31 elements or more", fn, n, (long long)px);
    NDET_REQUIRE((((uintptr_t)da | (uintptr_t)db) & 1) == 0 && ((uintptr_t)out & 7) == 0, NDET_E_UNSUPPORTED,
                 "%s: the depth frames must be 2-byte aligned, out 8-byte aligned", fn);
    const hipError_t e = hipMemsetAsync(out, 0, (size_t)n * 4 * sizeof(int64_t), (hipStream_t)stream);
    NDET_REQUIRE(e == hipSuccess, NDET_E_LAUNCH, "%s: cannot clear the sums: %s", fn, hipGetErrorString(e));
    const int bpf = (int)((px + 255) / 256);
    hipLaunchKernelGGL(k_frame_errors, dim3((unsigned)((int64_t)n * bpf)), dim3(256), 0, (hipStream_t)stream, a, b, da, db, (int)px, bpf,
                       reinterpret_cast<unsigned long long*>(out));
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}
