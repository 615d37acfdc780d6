// Tap positions of datasets.imresize_linear (cv2.INTER_LINEAR's geometry, resize.cpp), shared by the uint8 colour resize
// (frame_kernels.hip) and the float64 depth resize (depth_frames_kernels.hip): for output index d of an axis resized n_src -> n_dst,
//   f = float32(float64((d + 0.5) * (n_src / n_dst) - 0.5)), s = floor(f), f -= s, and both border clamps with f = 0
// (only an upscale reaches them).  n_src == n_dst gives s = d, f = 0: the copy.
#pragma once

struct FramePos {
    int s0, s1;   // source index of the two taps
    float f;      // weight of the second tap, in [0, 1); the first tap's is 1 - f in the caller's own precision
};

__device__ __forceinline__ FramePos frame_pos(int d, double scale /* n_src / n_dst */, int n_src) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f = f - (float)s;
    if (s < 0) { f = 0.0f; s = 0; }
    if (s >= n_src - 1) { f = 0.0f; s = n_src - 1; }
    FramePos p;
    p.s0 = s;
    p.s1 = s + 1 < n_src ? s + 1 : n_src - 1;
    p.f = f;
    return p;
}
