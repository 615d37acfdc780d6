// Detections out: the 3D boxes of detect() in the space the camera server works in -- where a box falls in a camera frame, its wireframe
// drawn onto a frame that already lies in device memory, and the detection each pixel of a depth frame belongs to.  The reference keeps
// its detections as DepthInstance3DBoxes (mmdet3d/core/bbox/structures/depth_box3d.py:46-84 gives their corners, imvoxel_head_v2.py:544
// wraps them) and has no device path for any of this.  Five kernels, plain vector stores, no global atomics.
//
//   k_project_boxes_w  k_project_boxes' body (one template) with one more output: the reciprocal camera z of every surviving edge's ends.
//   k_draw_overlay   k_draw_boxes with a depth test of every covered pixel against a millimetre depth frame and with text plates above the
//       boxes' rectangles, both optional; 7 844 bytes of LDS, still the 32-wave cap that bounds the occupancy.
//   k_project_boxes  one thread per (pose, box): the 8 corners through a world-to-camera matrix, each of the 12 edges clipped at the near
//       plane, its ends as output pixels of the (x0, y0, stride) grid of k_camera_rays (frames_out_kernels.hip), the bounding rectangle of
//       what survives inside the frame and the camera-z range.  Float32 in one fixed statement order (include/nerfdet_hip.h); every fused
//       step is an explicit fmaf (the library is built with -ffp-contract=off).
//   k_draw_boxes     one workgroup per 16 x 16 tile of one frame: a gather.  The workgroup walks the frame's 12 n edges in batches of 256,
//       keeps in LDS those whose bounding box -- grown by the line's radius across the major axis -- meets the tile, and every thread then
//       tests its pixel against the kept edges with the integer line rule and keeps the LARGEST box index: the same bytes in any order.
//       5 KiB of LDS a workgroup, so the 32-wave cap of a CU (8 workgroups) bounds the occupancy, not the LDS.
//   k_label_frames   one thread per pixel of a uint16 millimetre depth frame: the pixel's point along k_camera_rays' own direction, turned
//       into each box's frame (boxes staged through LDS, 256 at a time); the highest index among the boxes that hold it, -1 for none.
#include "ndet_common.hpp"

#define DO_TILE 16
#define DO_BATCH 256
#define DO_CLAMP 1048576.0f   // 2^20: keeps 2 * b * (x - x_a) + a of the line rule far inside int64

// camera point -> output pixel coordinate before the floor; u = fmaf(f, c / z, centre), then the grid's offset and stride
__device__ __forceinline__ float do_pixel(float f, float centre, float c, float z, int off, int stride) {
    const float u = fmaf(f, c / z, centre);
    return (u - ((float)off + 0.5f)) / (float)stride + 0.5f;
}

__device__ __forceinline__ int do_cell(float v) {
    return (int)floorf(fminf(fmaxf(v, -DO_CLAMP), DO_CLAMP));
}

// the body of k_project_boxes and k_project_boxes_w: WITH_W adds the reciprocal camera z of every surviving edge's ends, after the clip
template <bool WITH_W>
__device__ __forceinline__ void do_project_boxes(const float* __restrict__ kn /* (2,3) */, const float* __restrict__ w2c /* (k,3,4) */,
                                                 const float* __restrict__ corners /* (n,8,3) */, int k, int n, int x0, int y0, int stride, int h,
                                                 int w, float near_m, int* __restrict__ edges, int* __restrict__ edge_mask, int* __restrict__ rect,
                                                 float* __restrict__ zrange, float* __restrict__ edge_w) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k * n) return;
    const int pose = i / n, box = i - pose * n;
    const float* E = w2c + (int64_t)pose * 12;
    const float* C = corners + (int64_t)box * 24;
    float cx[8], cy[8], cz[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float X = C[c * 3 + 0], Y = C[c * 3 + 1], Z = C[c * 3 + 2];
        float q[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) q[r] = fmaf(E[r * 4 + 2], Z, fmaf(E[r * 4 + 1], Y, E[r * 4 + 0] * X)) + E[r * 4 + 3];
        cx[c] = q[0], cy[c] = q[1], cz[c] = q[2];
    }
    float zmin = cz[0], zmax = cz[0];
#pragma unroll
    for (int c = 1; c < 8; ++c) {
        if (cz[c] < zmin || zmin != zmin) zmin = cz[c];
        if (cz[c] > zmax || zmax != zmax) zmax = cz[c];
    }
    zrange[(int64_t)i * 2 + 0] = zmin;
    zrange[(int64_t)i * 2 + 1] = zmax;

    // the 12 edges as corner pairs: the x = 0 face loop, the x = 1 face loop, the four connectors
    constexpr int edge_a[12] = {0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3}, edge_b[12] = {1, 2, 3, 0, 5, 6, 7, 4, 4, 5, 6, 7};
    int mask = 0, xmin = INT32_MAX, ymin = INT32_MAX, xmax = INT32_MIN, ymax = INT32_MIN;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        const int a = edge_a[e], b = edge_b[e];
        float ax = cx[a], ay = cy[a], az = cz[a], bx = cx[b], by = cy[b], bz = cz[b];
        const bool oka = az >= near_m, okb = bz >= near_m;     // a NaN fails
        int4 out = make_int4(0, 0, 0, 0);
        float2 rz = make_float2(0.0f, 0.0f);
        if (oka || okb) {
            if (!okb) {                                        // b moves to the near plane along the edge from a
                const float t = (near_m - az) / (bz - az);
                bx = fmaf(t, bx - ax, ax), by = fmaf(t, by - ay, ay), bz = near_m;
            } else if (!oka) {
                const float t = (near_m - bz) / (az - bz);
                ax = fmaf(t, ax - bx, bx), ay = fmaf(t, ay - by, by), az = near_m;
            }
            const float xa = do_pixel(kn[0], kn[2], ax, az, x0, stride), ya = do_pixel(kn[4], kn[5], ay, az, y0, stride);
            const float xb = do_pixel(kn[0], kn[2], bx, bz, x0, stride), yb = do_pixel(kn[4], kn[5], by, bz, y0, stride);
            if (xa == xa && ya == ya && xb == xb && yb == yb) {
                out = make_int4(do_cell(xa), do_cell(ya), do_cell(xb), do_cell(yb));
                mask |= 1 << e;
                if (WITH_W) rz = make_float2(1.0f / az, 1.0f / bz);
                xmin = min(xmin, min(out.x, out.z)), xmax = max(xmax, max(out.x, out.z));
                ymin = min(ymin, min(out.y, out.w)), ymax = max(ymax, max(out.y, out.w));
            }
        }
        reinterpret_cast<int4*>(edges)[(int64_t)i * 12 + e] = out;
        if (WITH_W) reinterpret_cast<float2*>(edge_w)[(int64_t)i * 12 + e] = rz;
    }
    edge_mask[i] = mask;
    xmin = max(xmin, 0), ymin = max(ymin, 0), xmax = min(xmax, w - 1), ymax = min(ymax, h - 1);
    const bool any = mask != 0 && xmin <= xmax && ymin <= ymax;
    reinterpret_cast<int4*>(rect)[i] = any ? make_int4(xmin, ymin, xmax, ymax) : make_int4(-1, -1, -1, -1);
}

__global__ __launch_bounds__(256) void k_project_boxes(const float* __restrict__ kn, const float* __restrict__ w2c, const float* __restrict__ corners, int k,
                                                       int n, int x0, int y0, int stride, int h, int w, float near_m, int* __restrict__ edges,
                                                       int* __restrict__ edge_mask, int* __restrict__ rect, float* __restrict__ zrange) {
    do_project_boxes<false>(kn, w2c, corners, k, n, x0, y0, stride, h, w, near_m, edges, edge_mask, rect, zrange, nullptr);
}

__global__ __launch_bounds__(256) void k_project_boxes_w(const float* __restrict__ kn, const float* __restrict__ w2c, const float* __restrict__ corners,
                                                         int k, int n, int x0, int y0, int stride, int h, int w, float near_m, int* __restrict__ edges,
                                                         int* __restrict__ edge_mask, int* __restrict__ rect, float* __restrict__ zrange,
                                                         float* __restrict__ edge_w /* (k,n,12,2) */) {
    do_project_boxes<true>(kn, w2c, corners, k, n, x0, y0, stride, h, w, near_m, edges, edge_mask, rect, zrange, edge_w);
}

// floor(num / den) for den > 0
__device__ __forceinline__ long long do_floor_div(long long num, long long den) {
    long long q = num / den;
    if (num % den != 0 && num < 0) --q;
    return q;
}

__global__ __launch_bounds__(256) void k_draw_boxes(const uint8_t* __restrict__ frames_in, const int* __restrict__ edges, const int* __restrict__ edge_mask,
                                                    const uint8_t* __restrict__ colours, int h, int w, int n, int radius, int tiles_x, int tiles_y,
                                                    uint8_t* __restrict__ frames_out) {
    // a kept edge: major-axis start and end (start <= end), the minor coordinate at either, and box << 1 | y_major
    __shared__ int4 s_edge[DO_BATCH];
    __shared__ int s_tag[DO_BATCH];
    __shared__ int s_count;
    const int tid = threadIdx.x;
    const int per_frame = tiles_x * tiles_y;
    const int f = blockIdx.x / per_frame;
    const int t = blockIdx.x - f * per_frame;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int X0 = tx * DO_TILE, Y0 = ty * DO_TILE;
    const int x = X0 + (tid & (DO_TILE - 1)), y = Y0 + (tid >> 4);
    const int n_edges = 12 * n;
    const int4* E = reinterpret_cast<const int4*>(edges) + (int64_t)f * n_edges;
    const int* M = edge_mask + (int64_t)f * n;
    int best = -1;
    for (int base = 0; base < n_edges; base += DO_BATCH) {
        if (tid == 0) s_count = 0;
        __syncthreads();
        const int idx = base + tid;
        if (idx < n_edges) {
            const int box = idx / 12, e = idx - box * 12;
            if ((M[box] >> e) & 1) {
                const int4 v = E[idx];
                const int a = v.z - v.x, b = v.w - v.y;
                const bool y_major = abs(a) < abs(b);
                int p0 = y_major ? v.y : v.x, q0 = y_major ? v.x : v.y, p1 = y_major ? v.w : v.z, q1 = y_major ? v.z : v.w;
                if (p0 > p1) {
                    int s = p0; p0 = p1, p1 = s;
                    s = q0, q0 = q1, q1 = s;
                }
                const int P0 = y_major ? Y0 : X0, Q0 = y_major ? X0 : Y0;      // the tile along the major and the minor axis
                const int qlo = min(q0, q1) - radius, qhi = max(q0, q1) + radius;
                if (p0 <= P0 + DO_TILE - 1 && p1 >= P0 && qlo <= Q0 + DO_TILE - 1 && qhi >= Q0) {
                    const int at = atomicAdd(&s_count, 1);                      // LDS; the order of the kept edges does not matter
                    s_edge[at] = make_int4(p0, q0, p1, q1);
                    s_tag[at] = (box << 1) | (y_major ? 1 : 0);
                }
            }
        }
        __syncthreads();
        const int kept = s_count;
        for (int j = 0; j < kept; ++j) {
            const int tag = s_tag[j];
            const int box = tag >> 1;
            if (box <= best) continue;
            const int4 v = s_edge[j];
            const int P = (tag & 1) ? y : x, Q = (tag & 1) ? x : y;
            if (P < v.x || P > v.z) continue;
            const long long a = (long long)v.z - v.x, b = (long long)v.w - v.y;
            const long long ql = a == 0 ? (long long)v.y : (long long)v.y + do_floor_div(2 * b * ((long long)P - v.x) + a, 2 * a);
            const long long d = (long long)Q - ql;
            if (d >= -radius && d <= radius) best = box;
        }
        __syncthreads();
    }
    if (x < w && y < h) {
        const int64_t at = (((int64_t)f * h + y) * w + x) * 3;
        const uint8_t* src = best >= 0 ? colours + best * 3 : frames_in + at;
#pragma unroll
        for (int c = 0; c < 3; ++c) frames_out[at + c] = src[c];
    }
}

// k_draw_boxes' gather with an optional depth test of every covered pixel (depth_mm + edge_w, both or neither) and optional text plates
// (rect + text + text_len + font, all or none); with neither it writes k_draw_boxes' bytes.  One workgroup per 16 x 16 tile.  First the
// plates of the frame's n boxes, 256 at a time: s_edge holds px0, py0, len, box of those that meet the tile, a pixel keeps the highest
// box.  Then the edges as in k_draw_boxes, their two 1/z in s_w ordered like their ends; a pixel under a plate only keeps the barriers.
__global__ __launch_bounds__(256) void k_draw_overlay(const uint8_t* __restrict__ frames_in, const int* __restrict__ edges, const int* __restrict__ edge_mask,
                                                      const uint8_t* __restrict__ colours, const uint16_t* __restrict__ depth_mm,
                                                      const float* __restrict__ edge_w, float bias_mm, int dim, const int* __restrict__ rect,
                                                      const uint8_t* __restrict__ text, const int* __restrict__ text_len, const uint8_t* __restrict__ font,
                                                      int scale, int h, int w, int n, int radius, int tiles_x, int tiles_y,
                                                      uint8_t* __restrict__ frames_out) {
    __shared__ int4 s_edge[DO_BATCH];
    __shared__ float2 s_w[DO_BATCH];
    __shared__ int s_tag[DO_BATCH];
    __shared__ uint8_t s_font[96 * 7];
    __shared__ int s_count;
    const int tid = threadIdx.x;
    const int per_frame = tiles_x * tiles_y;
    const int f = blockIdx.x / per_frame;
    const int t = blockIdx.x - f * per_frame;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int X0 = tx * DO_TILE, Y0 = ty * DO_TILE;
    const int x = X0 + (tid & (DO_TILE - 1)), y = Y0 + (tid >> 4);
    const bool inside = x < w && y < h;

    int plate = -1, pu = 0, pv = 0, plen = 0;                  // the pixel's plate: its box, the pixel's cell in it, the text's length
    if (rect != nullptr) {
        for (int j = tid; j < 96 * 7; j += 256) s_font[j] = font[j];   // read behind the barriers below (n >= 1)
        const int ph = scale * 9;
        for (int base = 0; base < n; base += DO_BATCH) {
            if (tid == 0) s_count = 0;
            __syncthreads();
            const int box = base + tid;
            if (box < n) {
                const int4 rc = reinterpret_cast<const int4*>(rect)[(int64_t)f * n + box];
                const int len = min(max(text_len[box], 0), 32);
                if (rc.x >= 0 && len > 0) {
                    const int pw = scale * (6 * len + 1);
                    const int px0 = min(rc.x, max(w - pw, 0)), py0 = max(rc.y - ph, 0);
                    if (px0 <= X0 + DO_TILE - 1 && px0 + pw > X0 && py0 <= Y0 + DO_TILE - 1 && py0 + ph > Y0) {
                        const int at = atomicAdd(&s_count, 1);      // LDS; the highest box wins in any order
                        s_edge[at] = make_int4(px0, py0, len, box);
                    }
                }
            }
            __syncthreads();
            const int kept = s_count;
            for (int j = 0; j < kept; ++j) {
                const int4 v = s_edge[j];
                if (v.w > plate && x >= v.x && x < v.x + scale * (6 * v.z + 1) && y >= v.y && y < v.y + ph)
                    plate = v.w, pu = (x - v.x) / scale, pv = (y - v.y) / scale, plen = v.z;
            }
            __syncthreads();
        }
    }

    const int mm = depth_mm != nullptr && inside ? depth_mm[((int64_t)f * h + y) * w + x] : 0;     // 0, a hole, hides nothing
    const float limit = (float)mm + bias_mm;
    const int n_edges = 12 * n;
    const int4* E = reinterpret_cast<const int4*>(edges) + (int64_t)f * n_edges;
    const float2* W = edge_w != nullptr ? reinterpret_cast<const float2*>(edge_w) + (int64_t)f * n_edges : nullptr;
    const int* M = edge_mask + (int64_t)f * n;
    int bv = -1, bh = -1;                                      // the highest box with a visible / with a hidden covering edge
    for (int base = 0; base < n_edges; base += DO_BATCH) {
        if (tid == 0) s_count = 0;
        __syncthreads();
        const int idx = base + tid;
        if (idx < n_edges) {
            const int box = idx / 12, e = idx - box * 12;
            if ((M[box] >> e) & 1) {
                const int4 v = E[idx];
                const int a = v.z - v.x, b = v.w - v.y;
                const bool y_major = abs(a) < abs(b);
                int p0 = y_major ? v.y : v.x, q0 = y_major ? v.x : v.y, p1 = y_major ? v.w : v.z, q1 = y_major ? v.z : v.w;
                const bool swapped = p0 > p1;
                if (swapped) {
                    int s = p0; p0 = p1, p1 = s;
                    s = q0, q0 = q1, q1 = s;
                }
                const int P0 = y_major ? Y0 : X0, Q0 = y_major ? X0 : Y0;
                const int qlo = min(q0, q1) - radius, qhi = max(q0, q1) + radius;
                if (p0 <= P0 + DO_TILE - 1 && p1 >= P0 && qlo <= Q0 + DO_TILE - 1 && qhi >= Q0) {
                    const int at = atomicAdd(&s_count, 1);
                    s_edge[at] = make_int4(p0, q0, p1, q1);
                    s_tag[at] = (box << 1) | (y_major ? 1 : 0);
                    if (edge_w != nullptr) {
                        const float2 rz = W[idx];                   // the ends' 1/z swap with the ends
                        s_w[at] = swapped ? make_float2(rz.y, rz.x) : rz;
                    }
                }
            }
        }
        __syncthreads();
        const int kept = plate < 0 ? s_count : 0;
        for (int j = 0; j < kept; ++j) {
            const int tag = s_tag[j];
            const int box = tag >> 1;
            if (box <= bv) continue;                            // a visible edge beats a hidden one of any index: bh no longer matters
            const int4 v = s_edge[j];
            const int P = (tag & 1) ? y : x, Q = (tag & 1) ? x : y;
            if (P < v.x || P > v.z) continue;
            const long long a = (long long)v.z - v.x, b = (long long)v.w - v.y;
            const long long ql = a == 0 ? (long long)v.y : (long long)v.y + do_floor_div(2 * b * ((long long)P - v.x) + a, 2 * a);
            const long long d = (long long)Q - ql;
            if (d < -radius || d > radius) continue;
            bool hidden = false;
            if (mm != 0) {
                const float2 rz = s_w[j];
                const float wp = a == 0 ? rz.x : fmaf((float)(P - v.x) / (float)(v.z - v.x), rz.y - rz.x, rz.x);
                const float e_mm = (1.0f / wp) * 1000.0f;
                hidden = limit < e_mm;
            }
            if (!hidden) bv = box;
            else if (box > bh) bh = box;                        // a hidden edge only moves bh, and only upwards
        }
        __syncthreads();
    }
    if (inside) {
        const int64_t at = (((int64_t)f * h + y) * w + x) * 3;
        uint8_t out[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = frames_in[at + c];
        if (plate >= 0) {
            const uint8_t* col = colours + plate * 3;
            const int c = pu - 1, r = pv - 1;
            bool ink = false;
            if (c >= 0 && r >= 0 && r <= 6) {
                const int g = c / 6, gc = c - 6 * g;
                if (gc < 5 && g < plen) {
                    const int code = text[plate * 32 + g];
                    const int glyph = code >= 32 && code <= 127 ? code - 32 : 95;
                    ink = (s_font[glyph * 7 + r] >> (4 - gc)) & 1;
                }
            }
            const uint8_t pen = ((29 * col[0] + 150 * col[1] + 77 * col[2] + 128) >> 8) >= 128 ? 0 : 255;   // BGR: black ink on a light plate
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) out[ch] = ink ? pen : col[ch];
        } else if (bv >= 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c] = colours[bv * 3 + c];
        } else if (dim && bh >= 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c] = (uint8_t)((3 * out[c] + colours[bh * 3 + c] + 2) >> 2);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) frames_out[at + c] = out[c];
    }
}

__global__ __launch_bounds__(256) void k_label_frames(const uint16_t* __restrict__ depth_mm, const float* __restrict__ kn /* (2,3) */,
                                                      const float* __restrict__ rot /* (k,3,3) */, const float* __restrict__ lpos /* (k,3) */,
                                                      const float* __restrict__ boxes /* (n,8) */, int px, int w, int n, int x0, int y0, int stride,
                                                      int blocks_per_frame, int16_t* __restrict__ labels) {
    const int f = blockIdx.x / blocks_per_frame;
    const int p = (blockIdx.x - f * blocks_per_frame) * 256 + threadIdx.x;
    const int64_t at = (int64_t)f * px + p;
    const int mm = p < px ? depth_mm[at] : 0;
    float pt[3] = {0.0f, 0.0f, 0.0f};
    if (mm != 0) {
        const int row = p / w, col = p - row * w;
        const float z = (float)mm / 1000.0f;
        float d[3];
        ndet_pixel_dir(kn, rot + (int64_t)f * 9, x0 + col * stride, y0 + row * stride, d);
#pragma unroll
        for (int j = 0; j < 3; ++j) pt[j] = ndet_ray_point(z, d[j], lpos[(int64_t)f * 3 + j]);
    }
    const int best = ndet_box_of_point(boxes, n, mm != 0, pt[0], pt[1], pt[2]);
    if (p < px) labels[at] = (int16_t)best;
}

// ndet_project_boxes and ndet_project_boxes_w: the same checks, the same launch shape; edge_w is null for the former
static int do_project_entry(const char* fn, bool with_w, const float* intrinsic_rows, const float* world2cam, const float* corners, int k, int n, int x0,
                            int y0, int stride, int h, int w, float near_m, int32_t* edges, int32_t* edge_mask, int32_t* rect, float* zrange,
                            float* edge_w, void* stream) {
    NDET_REQUIRE(intrinsic_rows && world2cam && corners && edges && edge_mask && rect && zrange && (edge_w || !with_w), NDET_E_INVALID,
                 "%s: null pointer", fn);
    NDET_REQUIRE(k > 0 && n > 0 && h > 0 && w > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    NDET_REQUIRE(stride >= 1 && x0 >= 0 && y0 >= 0, NDET_E_INVALID, "%s: stride %d must be at least 1 and the offsets (%d, %d) non-negative", fn, stride,
                 x0, y0);
    NDET_REQUIRE(near_m > 0.0f, NDET_E_INVALID, "%s: near = %g must be positive", fn, (double)near_m);
    NDET_REQUIRE((((uintptr_t)intrinsic_rows | (uintptr_t)world2cam | (uintptr_t)corners | (uintptr_t)edge_mask | (uintptr_t)zrange) & 3) == 0 &&
                     (((uintptr_t)edges | (uintptr_t)rect) & 15) == 0,
                 NDET_E_UNSUPPORTED, "%s: pointers must be 4-byte aligned, edges and rect 16-byte aligned", fn);
    NDET_REQUIRE(((uintptr_t)edge_w & 7) == 0, NDET_E_UNSUPPORTED, "%s: edge_w must be 8-byte aligned", fn);
    NDET_REQUIRE((int64_t)k * n * 48 < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: %d poses of %d boxes hold 2^31 edge elements or more", fn, k, n);
    const int total = k * n;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (with_w)
        hipLaunchKernelGGL(k_project_boxes_w, grid, dim3(256), 0, (hipStream_t)stream, intrinsic_rows, world2cam, corners, k, n, x0, y0, stride, h, w,
                           near_m, edges, edge_mask, rect, zrange, edge_w);
    else
        hipLaunchKernelGGL(k_project_boxes, grid, dim3(256), 0, (hipStream_t)stream, intrinsic_rows, world2cam, corners, k, n, x0, y0, stride, h, w,
                           near_m, edges, edge_mask, rect, zrange);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_project_boxes(const float* intrinsic_rows, const float* world2cam, const float* corners, int k, int n, int x0, int y0, int stride,
                                  int h, int w, float near_m, int32_t* edges, int32_t* edge_mask, int32_t* rect, float* zrange, void* stream) {
    return do_project_entry("ndet_project_boxes", false, intrinsic_rows, world2cam, corners, k, n, x0, y0, stride, h, w, near_m, edges, edge_mask, rect,
                            zrange, nullptr, stream);
}

extern "C" int ndet_project_boxes_w(const float* intrinsic_rows, const float* world2cam, const float* corners, int k, int n, int x0, int y0, int stride,
                                    int h, int w, float near_m, int32_t* edges, int32_t* edge_mask, int32_t* rect, float* zrange, float* edge_w,
                                    void* stream) {
    return do_project_entry("ndet_project_boxes_w", true, intrinsic_rows, world2cam, corners, k, n, x0, y0, stride, h, w, near_m, edges, edge_mask, rect,
                            zrange, edge_w, stream);
}

extern "C" int ndet_draw_boxes(const uint8_t* frames_in, const int32_t* edges, const int32_t* edge_mask, const uint8_t* colours, int k, int h, int w,
                               int n, int thickness, uint8_t* frames_out, void* stream) {
    const char* fn = "ndet_draw_boxes";
    NDET_REQUIRE(frames_in && edges && edge_mask && colours && frames_out, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(k > 0 && h > 0 && w > 0 && n > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    NDET_REQUIRE(thickness == 1 || thickness == 3 || thickness == 5, NDET_E_INVALID, "%s: thickness %d is not 1, 3 or 5", fn, thickness);
    const int64_t two31 = (int64_t)1 << 31;
    NDET_REQUIRE((int64_t)k * h * w * 3 < two31, NDET_E_UNSUPPORTED, "%s: %d frames of %d x %d pixels hold 2^31 elements or more", fn, k, h, w);
    NDET_REQUIRE((int64_t)k * n * 48 < two31, NDET_E_UNSUPPORTED, "%s: %d frames of %d boxes hold 2^31 edge elements or more", fn, k, n);
    NDET_REQUIRE(((uintptr_t)edges & 15) == 0 && ((uintptr_t)edge_mask & 3) == 0, NDET_E_UNSUPPORTED,
                 "%s: edges must be 16-byte aligned, edge_mask 4-byte aligned", fn);
    const int64_t bytes = (int64_t)k * h * w * 3;
    const uintptr_t a = (uintptr_t)frames_in, b = (uintptr_t)frames_out;
    NDET_REQUIRE(a + (uintptr_t)bytes <= b || b + (uintptr_t)bytes <= a, NDET_E_INVALID, "%s: frames_out overlaps frames_in (the input is only read)", fn);
    const int tiles_x = (w + DO_TILE - 1) / DO_TILE, tiles_y = (h + DO_TILE - 1) / DO_TILE;
    NDET_REQUIRE((int64_t)k * tiles_x * tiles_y < ((int64_t)1 << 24), NDET_E_UNSUPPORTED, "%s: %d frames of %d x %d tiles make 2^24 workgroups or more", fn,
                 k, tiles_x, tiles_y);
    hipLaunchKernelGGL(k_draw_boxes, dim3((unsigned)((int64_t)k * tiles_x * tiles_y)), dim3(256), 0, (hipStream_t)stream, frames_in, edges, edge_mask,
                       colours, h, w, n, (thickness - 1) / 2, tiles_x, tiles_y, frames_out);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_draw_overlay(const uint8_t* frames_in, const int32_t* edges, const int32_t* edge_mask, const uint8_t* colours,
                                 const uint16_t* depth_mm, const float* edge_w, float bias_mm, int occluded, const int32_t* rect, const uint8_t* text,
                                 const int32_t* text_len, const uint8_t* font, int text_scale, int k, int h, int w, int n, int thickness,
                                 uint8_t* frames_out, void* stream) {
    const char* fn = "ndet_draw_overlay";
    NDET_REQUIRE(frames_in && edges && edge_mask && colours && frames_out, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE((depth_mm != nullptr) == (edge_w != nullptr), NDET_E_INVALID, "%s: depth_mm and edge_w come together or not at all", fn);
    const bool plates = rect != nullptr;
    NDET_REQUIRE((text != nullptr) == plates && (text_len != nullptr) == plates && (font != nullptr) == plates, NDET_E_INVALID,
                 "%s: rect, text, text_len and font come together or not at all", fn);
    NDET_REQUIRE(k > 0 && h > 0 && w > 0 && n > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    NDET_REQUIRE(thickness == 1 || thickness == 3 || thickness == 5, NDET_E_INVALID, "%s: thickness %d is not 1, 3 or 5", fn, thickness);
    NDET_REQUIRE(occluded == 0 || occluded == 1, NDET_E_INVALID, "%s: occluded %d is not 0 (hide) or 1 (dim)", fn, occluded);
    NDET_REQUIRE(std::isfinite(bias_mm) && bias_mm >= 0.0f, NDET_E_INVALID, "%s: bias_mm = %g must be finite and not negative", fn, (double)bias_mm);
    NDET_REQUIRE(!plates || (text_scale >= 1 && text_scale <= 3), NDET_E_INVALID, "%s: text_scale %d is not 1, 2 or 3", fn, text_scale);
    const int64_t two31 = (int64_t)1 << 31;
    NDET_REQUIRE((int64_t)k * h * w * 3 < two31, NDET_E_UNSUPPORTED, "%s: %d frames of %d x %d pixels hold 2^31 elements or more", fn, k, h, w);
    NDET_REQUIRE((int64_t)k * n * 48 < two31, NDET_E_UNSUPPORTED, "%s: %d frames of %d boxes hold 2^31 edge elements or more", fn, k, n);
    NDET_REQUIRE(((uintptr_t)edges & 15) == 0 && ((uintptr_t)edge_mask & 3) == 0, NDET_E_UNSUPPORTED,
                 "%s: edges must be 16-byte aligned, edge_mask 4-byte aligned", fn);
    NDET_REQUIRE(((uintptr_t)depth_mm & 1) == 0 && ((uintptr_t)edge_w & 7) == 0 && ((uintptr_t)rect & 15) == 0 && ((uintptr_t)text_len & 3) == 0,
                 NDET_E_UNSUPPORTED, "%s: depth_mm must be 2-byte aligned, edge_w 8-byte, rect 16-byte, text_len 4-byte", fn);
    const int64_t bytes = (int64_t)k * h * w * 3;
    const uintptr_t a = (uintptr_t)frames_in, b = (uintptr_t)frames_out;
    NDET_REQUIRE(a + (uintptr_t)bytes <= b || b + (uintptr_t)bytes <= a, NDET_E_INVALID, "%s: frames_out overlaps frames_in (the input is only read)", fn);
    const int tiles_x = (w + DO_TILE - 1) / DO_TILE, tiles_y = (h + DO_TILE - 1) / DO_TILE;
    NDET_REQUIRE((int64_t)k * tiles_x * tiles_y < ((int64_t)1 << 24), NDET_E_UNSUPPORTED, "%s: %d frames of %d x %d tiles make 2^24 workgroups or more", fn,
                 k, tiles_x, tiles_y);
    hipLaunchKernelGGL(k_draw_overlay, dim3((unsigned)((int64_t)k * tiles_x * tiles_y)), dim3(256), 0, (hipStream_t)stream, frames_in, edges, edge_mask,
                       colours, depth_mm, edge_w, bias_mm, occluded, rect, text, text_len, font, text_scale, h, w, n, (thickness - 1) / 2, tiles_x, tiles_y,
                       frames_out);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_label_frames(const uint16_t* depth_mm, const float* intrinsic_rows, const float* camrotc2w, const float* cam_lightpos,
                                 const float* box_frames, int k, int h, int w, int n, int x0, int y0, int stride, int16_t* labels, void* stream) {
    const char* fn = "ndet_label_frames";
    NDET_REQUIRE(depth_mm && intrinsic_rows && camrotc2w && cam_lightpos && box_frames && labels, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(k > 0 && h > 0 && w > 0 && n > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    NDET_REQUIRE(stride >= 1 && x0 >= 0 && y0 >= 0, NDET_E_INVALID, "%s: stride %d must be at least 1 and the offsets (%d, %d) non-negative", fn, stride,
                 x0, y0);
    NDET_REQUIRE(n <= 32767, NDET_E_UNSUPPORTED, "%s: %d boxes do not fit an int16 label", fn, n);
    const int64_t two31 = (int64_t)1 << 31;
    NDET_REQUIRE((int64_t)k * h * w < two31, NDET_E_UNSUPPORTED, "%s: %d frames of %d x %d pixels hold 2^31 elements or more", fn, k, h, w);
    NDET_REQUIRE(x0 + (int64_t)(w - 1) * stride < two31 && y0 + (int64_t)(h - 1) * stride < two31, NDET_E_UNSUPPORTED,
                 "%s: the last pixel lies at 2^31 or beyond", fn);
    NDET_REQUIRE((((uintptr_t)intrinsic_rows | (uintptr_t)camrotc2w | (uintptr_t)cam_lightpos | (uintptr_t)box_frames) & 3) == 0 &&
                     (((uintptr_t)depth_mm | (uintptr_t)labels) & 1) == 0,
                 NDET_E_UNSUPPORTED, "%s: float pointers must be 4-byte aligned, depth_mm and labels 2-byte aligned", fn);
    const int px = h * w;
    const int bpf = (px + 255) / 256;
    NDET_REQUIRE((int64_t)k * bpf < ((int64_t)1 << 24), NDET_E_UNSUPPORTED, "%s: %d frames of %d workgroups make 2^24 workgroups or more", fn, k, bpf);
    hipLaunchKernelGGL(k_label_frames, dim3((unsigned)((int64_t)k * bpf)), dim3(256), 0, (hipStream_t)stream, depth_mm, intrinsic_rows, camrotc2w,
                       cam_lightpos, box_frames, px, w, n, x0, y0, stride, bpf, labels);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}
