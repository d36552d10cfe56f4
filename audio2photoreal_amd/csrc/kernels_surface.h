// Surface maps of the posed body mesh (audio2photoreal_amd/surface.py): the second stage of the reference's renderer, visualize/
// ca_body/utils/geom.py -- vert_normals, compute_view_cos, values_to_uv, sample_uv as GeometryModule.from_uv calls it, and the
// UV index / barycentric images the reference gets from pytorch3d's rasteriser.  fp32 like the reference; every sum runs in a
// fixed order, the only atomic is an integer minimum (order-independent), and a frame's result depends on neither N nor its index.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#define SURFACE_MAX_UV 16384        // 3 H H stays below 2^31
#define SURFACE_MAX_CHANNELS 16
#define SURFACE_THREADS 256
#define SURFACE_FRAME_GROUP 8       // frames one thread of surface_to_uv_kernel writes for its texel

// The reference's length rule (face_normals / vert_normals): a length below 1e-5 counts as 1.
__device__ __forceinline__ float surface_safe_len(float x, float y, float z) {
  const float len = sqrtf(x * x + y * y + z * z);
  return len < 1e-5f ? 1.0f : len;
}

// Grid tiles * N (tiles = ceil(V / SURFACE_THREADS); block b is tile b % tiles of frame b / tiles): one thread per vertex and
// frame.  The thread walks its incidence range inc_face[inc_ptr[v] .. inc_ptr[v + 1]) (ascending face, then corner), recomputes
// each face's normalised normal from the frame's vertices and sums them in that order -- the order of the reference's
// scatter_add_ on the CPU -- then applies the length rule again.  With a camera: view_cos = normalize(vn) . normalize(p - cam),
// both with F.normalize's max(length, 1e-12).  normals [N, V, 3] and view_cos [N, V]; either may be NULL.
__global__ __launch_bounds__(SURFACE_THREADS) void surface_normals_kernel(
    const float* __restrict__ verts, int V, int tiles, const int* __restrict__ vi, const int* __restrict__ inc_ptr,
    const int* __restrict__ inc_face, const float* __restrict__ camera, int64_t camera_stride, float* __restrict__ normals,
    float* __restrict__ view_cos) {
  const int64_t n = blockIdx.x / tiles;
  const int v = (blockIdx.x % tiles) * SURFACE_THREADS + threadIdx.x;
  if (v >= V) return;
  const float* p = verts + n * V * 3;
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  const int end = inc_ptr[v + 1];
  for (int e = inc_ptr[v]; e < end; ++e) {
    const int* f = vi + 3 * (int64_t)inc_face[e];
    const float* p0 = p + 3 * (int64_t)f[0];
    const float* p1 = p + 3 * (int64_t)f[1];
    const float* p2 = p + 3 * (int64_t)f[2];
    const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
    const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
    const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const float len = surface_safe_len(nx, ny, nz);
    sx += nx / len;
    sy += ny / len;
    sz += nz / len;
  }
  const float len = surface_safe_len(sx, sy, sz);
  const float vx = sx / len, vy = sy / len, vz = sz / len;
  const int64_t o = n * V + v;
  if (normals) {
    normals[3 * o] = vx;
    normals[3 * o + 1] = vy;
    normals[3 * o + 2] = vz;
  }
  if (view_cos) {
    const float* c = camera + n * camera_stride;
    const float la = fmaxf(sqrtf(vx * vx + vy * vy + vz * vz), 1e-12f);
    const float dx = p[3 * (int64_t)v] - c[0], dy = p[3 * (int64_t)v + 1] - c[1], dz = p[3 * (int64_t)v + 2] - c[2];
    const float ld = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-12f);
    view_cos[o] = (vx / la) * (dx / ld) + (vy / la) * (dy / ld) + (vz / la) * (dz / ld);
  }
}

// Grid tblocks * groups (tblocks = ceil(H H / SURFACE_THREADS), groups = ceil(N / SURFACE_FRAME_GROUP); block b is texel block
// b % tblocks of frame group b / tblocks).  A thread owns one texel: it loads the texel's three indices and barycentrics once and
// writes the texel of every channel plane of its group's frames -- values_to_uv:
//   out[n][c][texel] = b0 x[n][i0][c] + b1 x[n][i1][c] + b2 x[n][i2][c]   when i0, i1, i2 all differ from -1, else 0
// Consecutive threads write consecutive texels of one plane; a frame's planes are written by its group alone, from its own
// values.  Every offset is 64-bit (N C H H exceeds 2^31 at workload sizes).
__global__ __launch_bounds__(SURFACE_THREADS) void surface_to_uv_kernel(
    const float* __restrict__ values, int64_t N, int V, int C, const int* __restrict__ index_image,
    const float* __restrict__ bary_image, int64_t HH, int64_t tblocks, float* __restrict__ out) {
  const int64_t t = (blockIdx.x % tblocks) * SURFACE_THREADS + threadIdx.x;
  if (t >= HH) return;
  const int64_t n0 = (blockIdx.x / tblocks) * SURFACE_FRAME_GROUP;
  const int64_t n1 = min(N, n0 + SURFACE_FRAME_GROUP);
  const int i0 = index_image[3 * t], i1 = index_image[3 * t + 1], i2 = index_image[3 * t + 2];
  const bool valid = i0 != -1 && i1 != -1 && i2 != -1;
  const float b0 = bary_image[3 * t], b1 = bary_image[3 * t + 1], b2 = bary_image[3 * t + 2];
  for (int64_t n = n0; n < n1; ++n) {
    const float* x = values + n * V * C;
    float* o = out + n * C * HH + t;
    if (valid) {
      const float* x0 = x + (int64_t)i0 * C;
      const float* x1 = x + (int64_t)i1 * C;
      const float* x2 = x + (int64_t)i2 * C;
      for (int c = 0; c < C; ++c) o[c * HH] = b0 * x0[c] + b1 * x1[c] + b2 * x2[c];
    } else {
      for (int c = 0; c < C; ++c) o[c * HH] = 0.0f;
    }
  }
}

// Grid tiles * N like surface_normals_kernel: one thread per vertex and frame, looping over the channels.  sample_uv(values_uv,
// vt, v2uv) as GeometryModule.from_uv calls it: for each of the vertex's 4 slots (v2uv [V, 4], padded slots repeat the first
// texture index and count again) the texture coordinate becomes a pixel coordinate by grid_sample's own float32 operations
// (align_corners = True):  g = 2 u - 1,  x = ((g + 1) / 2) (W - 1),  likewise y with H;  the four taps nw, ne, sw, se are
// weighted (1 - fy)(1 - fx), (1 - fy) fx, fy (1 - fx), fy fx and summed in that order, a tap outside the image counting 0;  the
// vertex value is the sum of the 4 slot samples in slot order, divided by 4.  values_uv [N, C, Hs, Ws] -> out [N, V, C].
__global__ __launch_bounds__(SURFACE_THREADS) void surface_from_uv_kernel(
    const float* __restrict__ values_uv, int C, int Hs, int Ws, const float* __restrict__ vt, const int* __restrict__ v2uv,
    int V, int tiles, float* __restrict__ out) {
  const int64_t n = blockIdx.x / tiles;
  const int v = (blockIdx.x % tiles) * SURFACE_THREADS + threadIdx.x;
  if (v >= V) return;
  int off[4][4];        // tap offsets inside one plane, -1 for a tap outside it
  float wt[4][4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float* uv = vt + 2 * (int64_t)v2uv[4 * (int64_t)v + s];
    const float gx = uv[0] * 2.0f - 1.0f, gy = uv[1] * 2.0f - 1.0f;
    const float x = ((gx + 1.0f) / 2.0f) * (float)(Ws - 1), y = ((gy + 1.0f) / 2.0f) * (float)(Hs - 1);
    const float xw = floorf(x), yn = floorf(y);
    const float w = x - xw, e = 1.0f - w, nn = y - yn, so = 1.0f - nn;
    wt[s][0] = so * e;
    wt[s][1] = so * w;
    wt[s][2] = nn * e;
    wt[s][3] = nn * w;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float xi = xw + (float)(k & 1), yi = yn + (float)(k >> 1);
      const bool in = xi >= 0.0f && xi <= (float)(Ws - 1) && yi >= 0.0f && yi <= (float)(Hs - 1);   // false for a NaN too
      off[s][k] = in ? (int)yi * Ws + (int)xi : -1;
    }
  }
  const int64_t plane = (int64_t)Hs * Ws;
  const float* img = values_uv + n * C * plane;
  float* o = out + (n * V + v) * C;
  for (int c = 0; c < C; ++c) {
    const float* p = img + c * plane;
    float sum = 0.0f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float a = (off[s][0] >= 0 ? p[off[s][0]] : 0.0f) * wt[s][0];
#pragma unroll
      for (int k = 1; k < 4; ++k) a += (off[s][k] >= 0 ? p[off[s][k]] : 0.0f) * wt[s][k];
      sum = s == 0 ? a : sum + a;
    }
    o[c] = sum / 4.0f;
  }
}

// ---- the one-time UV rasterisation ------------------------------------------------------------------------------------------
// The texel at row i, column j has centre ((j + 0.5) / H, (i + 0.5) / H).  A face covers it when the centre is inside or on the
// boundary of the face's UV triangle (all three edge functions >= 0 or all <= 0); a zero-area triangle covers nothing; of
// several covering faces the lowest index wins.
__device__ __forceinline__ float surface_texel_centre(int k, int H) { return ((float)k + 0.5f) / (float)H; }

__global__ __launch_bounds__(SURFACE_THREADS) void surface_fill_kernel(int* __restrict__ p, int64_t n, int value) {
  const int64_t i = (int64_t)blockIdx.x * SURFACE_THREADS + threadIdx.x;
  if (i < n) p[i] = value;
}

// Pass A.  Grid ceil(F / 4), SURFACE_THREADS threads: one wave per face.  The wave's lanes stride over the texels of the face's
// bounding box (clipped to the image, widened by one texel so that float rounding of the box cannot lose a texel: the edge
// functions decide) and apply an integer atomicMin of the face index to face_image (initialised to INT_MAX).
__global__ __launch_bounds__(SURFACE_THREADS) void surface_uv_cover_kernel(
    const float* __restrict__ vt, const int* __restrict__ vti, int F, int H, int* __restrict__ face_image) {
  const int f = blockIdx.x * (SURFACE_THREADS / 64) + threadIdx.x / 64;
  if (f >= F) return;
  const int lane = threadIdx.x % 64;
  const float* a = vt + 2 * (int64_t)vti[3 * (int64_t)f];
  const float* b = vt + 2 * (int64_t)vti[3 * (int64_t)f + 1];
  const float* c = vt + 2 * (int64_t)vti[3 * (int64_t)f + 2];
  const float ax = a[0], ay = a[1], bx = b[0], by = b[1], cx = c[0], cy = c[1];
  const float area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
  if (!(fabsf(area) > 0.0f)) return;                             // zero area (or a NaN): covers nothing
  // clamp in float first: a coordinate far outside [0, 1] must not overflow the conversion
  const float fH = (float)H;
  const float ulo = fminf(fmaxf(fminf(fminf(ax, bx), cx) * fH, -2.0f), fH + 2.0f);
  const float uhi = fminf(fmaxf(fmaxf(fmaxf(ax, bx), cx) * fH, -2.0f), fH + 2.0f);
  const float vlo = fminf(fmaxf(fminf(fminf(ay, by), cy) * fH, -2.0f), fH + 2.0f);
  const float vhi = fminf(fmaxf(fmaxf(fmaxf(ay, by), cy) * fH, -2.0f), fH + 2.0f);
  const int j0 = max(0, (int)floorf(ulo - 0.5f) - 1), j1 = min(H - 1, (int)ceilf(uhi - 0.5f) + 1);
  const int i0 = max(0, (int)floorf(vlo - 0.5f) - 1), i1 = min(H - 1, (int)ceilf(vhi - 0.5f) + 1);
  if (j1 < j0 || i1 < i0) return;
  const int bw = j1 - j0 + 1;
  const int64_t count = (int64_t)bw * (i1 - i0 + 1);
  for (int64_t t = lane; t < count; t += 64) {
    const int i = i0 + (int)(t / bw), j = j0 + (int)(t % bw);
    const float px = surface_texel_centre(j, H), py = surface_texel_centre(i, H);
    const float w0 = (bx - ax) * (py - ay) - (by - ay) * (px - ax);
    const float w1 = (cx - bx) * (py - by) - (cy - by) * (px - bx);
    const float w2 = (ax - cx) * (py - cy) - (ay - cy) * (px - cx);
    if ((w0 >= 0.0f && w1 >= 0.0f && w2 >= 0.0f) || (w0 <= 0.0f && w1 <= 0.0f && w2 <= 0.0f))
      atomicMin(face_image + (int64_t)i * H + j, f);
  }
}

// Pass B.  One thread per texel: no face -> index -1, barycentrics 0, face -1; otherwise index = vi[face] and the barycentrics of
// the texel centre by the reference's bary_coords in float32 (denominator kept at least 1e-6 from 0 on its own side).
__global__ __launch_bounds__(SURFACE_THREADS) void surface_uv_resolve_kernel(
    const float* __restrict__ vt, const int* __restrict__ vti, const int* __restrict__ vi, int H, int* __restrict__ index_image,
    float* __restrict__ bary_image, int* __restrict__ face_image) {
  const int64_t t = (int64_t)blockIdx.x * SURFACE_THREADS + threadIdx.x;
  if (t >= (int64_t)H * H) return;
  const int f = face_image[t];
  if (f == INT_MAX) {
    face_image[t] = -1;
    for (int k = 0; k < 3; ++k) {
      index_image[3 * t + k] = -1;
      bary_image[3 * t + k] = 0.0f;
    }
    return;
  }
  const float px = surface_texel_centre((int)(t % H), H), py = surface_texel_centre((int)(t / H), H);
  const float* t0 = vt + 2 * (int64_t)vti[3 * (int64_t)f];
  const float* t1 = vt + 2 * (int64_t)vti[3 * (int64_t)f + 1];
  const float* t2 = vt + 2 * (int64_t)vti[3 * (int64_t)f + 2];
  const float x = px - t2[0], x1 = t0[0] - t2[0], x2 = t1[0] - t2[0];
  const float y = py - t2[1], y1 = t0[1] - t2[1], y2 = t1[1] - t2[1];
  float denom = y2 * x1 - y1 * x2;
  const float n0 = y2 * x - x2 * y, n1 = x1 * y - y1 * x;
  denom = denom >= 0.0f ? fmaxf(denom, 1e-6f) : fminf(denom, -1e-6f);
  const float b0 = n0 / denom, b1 = n1 / denom;
  bary_image[3 * t] = b0;
  bary_image[3 * t + 1] = b1;
  bary_image[3 * t + 2] = 1.0f - b0 - b1;
  for (int k = 0; k < 3; ++k) index_image[3 * t + k] = vi[3 * (int64_t)f + k];
}
