// Rendered images of the posed body mesh (audio2photoreal_amd/render.py): the third stage of the reference's renderer, visualize/
// ca_body/utils/render.py RenderLayer -- what it gets from pytorch3d's MeshRasterizer (faces_per_pixel = 1, blur_radius = 0, no
// culling, perspective-correct barycentrics) and TexturesUV.sample_textures.  fp32 like the reference; all frames of a call in a
// fixed number of launches; the only atomic is a 64-bit integer minimum (order-independent), so two runs give the same bits and a
// frame's result depends on neither N nor its index.  Every offset into an [N, ...] array is 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RENDER_MAX_SIZE 8192
#define RENDER_MAX_CHANNELS 16
#define RENDER_THREADS 256
#ifndef RENDER_SMALL_BOX            // -DRENDER_SMALL_BOX=0: every face takes the wave path (the A/B of DESIGN.md's measurement)
#define RENDER_SMALL_BOX 64         // a face whose clipped box holds at most this many pixels is walked by its own thread
#endif
#define RENDER_EMPTY_KEY 0xffffffffffffffffull

// Pass 0.  Grid tiles * N (tiles = ceil(V / RENDER_THREADS)): one thread per vertex and frame.  p = R x + t with Rt [., 3, 4];
// u = fx (x / z) + skew (y / z) + cx, v = fy (y / z) + cy with K [., 3, 3] (K[0][0], K[0][1], K[0][2], K[1][1], K[1][2]); proj
// [N, V, 3] keeps (u, v, z).  A vertex at z <= 0 gives values no later pass reads: its faces fail the near test first.
// One vertex through Rt (m, 12 floats) and the five entries of K that are read.
__device__ __forceinline__ void render_project_vertex(const float* __restrict__ verts, const float* __restrict__ m, float k0, float k1,
                                                      float k2, float k4, float k5, int64_t o, float* __restrict__ proj) {
#pragma clang fp contract(off)      // sums left to right as written: which pixels a face covers hangs on these coordinates
  const float x = verts[o], y = verts[o + 1], z = verts[o + 2];
  const float xc = m[0] * x + m[1] * y + m[2] * z + m[3];
  const float yc = m[4] * x + m[5] * y + m[6] * z + m[7];
  const float zc = m[8] * x + m[9] * y + m[10] * z + m[11];
  const float xn = xc / zc, yn = yc / zc;
  proj[o] = k0 * xn + k1 * yn + k2;
  proj[o + 1] = k4 * yn + k5;
  proj[o + 2] = zc;
}

// k * scale is one float32 multiplication: scale = S gives K' = K with its first two rows times S, the camera of the S H x S W sample
// grid (kernels_render_aa.h), the same bits as a K' the caller had scaled in float32; scale = 1 changes no bit (the plain rasteriser).
__global__ __launch_bounds__(RENDER_THREADS) void render_project_scaled_kernel(
    const float* __restrict__ verts, int V, int tiles, const float* __restrict__ K, int64_t k_stride,
    const float* __restrict__ Rt, int64_t rt_stride, float scale, float* __restrict__ proj) {
  const int64_t n = blockIdx.x / tiles;
  const int v = (blockIdx.x % tiles) * RENDER_THREADS + threadIdx.x;
  if (v >= V) return;
  const float* k = K + n * k_stride;
  render_project_vertex(verts, Rt + n * rt_stride, k[0] * scale, k[1] * scale, k[2] * scale, k[4] * scale, k[5] * scale,
                        3 * (n * V + v), proj);
}

// One projected face: corners (u, v, z) and twice its signed screen area.
struct RenderFace {
  float ax, ay, az, bx, by, bz, cx, cy, cz, area;
};

__device__ __forceinline__ RenderFace render_load_face(const float* __restrict__ p, const int* __restrict__ f) {
  const float* a = p + 3 * (int64_t)f[0];
  const float* b = p + 3 * (int64_t)f[1];
  const float* c = p + 3 * (int64_t)f[2];
  RenderFace t;
  t.ax = a[0], t.ay = a[1], t.az = a[2];
  t.bx = b[0], t.by = b[1], t.bz = b[2];
  t.cx = c[0], t.cy = c[1], t.cz = c[2];
  {
#pragma clang fp contract(off)
    t.area = (t.bx - t.ax) * (t.cy - t.ay) - (t.by - t.ay) * (t.cx - t.ax);
  }
  return t;
}

// The pixel at row i, column j has centre (j + 0.5, i + 0.5).  Edge functions w0 (edge a-b, the weight of c), w1 (b-c, of a), w2
// (c-a, of b); the centre is covered when all three are >= 0 or all <= 0.  q_k = w_k / z of the weighted corner, s = qa + qb + qc:
// the perspective-correct barycentrics are q / s and the depth is area / s (1 / z = sum of b_k / z_k with b_k = w_k / area).
// Without contraction, so that the cover pass and the resolve pass (separately compiled loops) compute the same bits.
__device__ __forceinline__ bool render_pixel(const RenderFace& t, int i, int j, float& qa, float& qb, float& qc, float& depth) {
#pragma clang fp contract(off)
  const float px = (float)j + 0.5f, py = (float)i + 0.5f;
  const float w0 = (t.bx - t.ax) * (py - t.ay) - (t.by - t.ay) * (px - t.ax);
  const float w1 = (t.cx - t.bx) * (py - t.by) - (t.cy - t.by) * (px - t.bx);
  const float w2 = (t.ax - t.cx) * (py - t.cy) - (t.ay - t.cy) * (px - t.cx);
  if (!((w0 >= 0.0f && w1 >= 0.0f && w2 >= 0.0f) || (w0 <= 0.0f && w1 <= 0.0f && w2 <= 0.0f))) return false;
  qa = w1 / t.az;
  qb = w2 / t.bz;
  qc = w0 / t.cz;
  depth = t.area / (qa + qb + qc);
  return depth > 0.0f && depth < __builtin_inff();                 // false for a NaN too: such a pixel is not covered
}

// The perspective-correct barycentrics q / s of a pixel (or sample) the face won: every resolve computes them here.
__device__ __forceinline__ void render_barycentrics(const RenderFace& t, int i, int j, float& b0, float& b1, float& b2) {
  float qa, qb, qc, d;
  render_pixel(t, i, j, qa, qb, qc, d);
  const float s = qa + qb + qc;
  b0 = qa / s, b1 = qb / s, b2 = qc / s;
}

// Where a uv falls in a texture plane [Ht, Wt]: the north-west texel (yi, xi), whether its east / south neighbours exist, and the
// weights of the taps nw, ne, sw, se: (1 - fy)(1 - fx), (1 - fy) fx, fy (1 - fx), fy fx of the position's fractions.
struct RenderTaps {
  int xi, yi;
  bool east, south;
  float nw, ne, sw, se;
};

// uv = b0 t0 + b1 t1 + b2 t2 (v <- 1 - v when flip_v); sample position x = u (Wt - 1), y = v (Ht - 1), clamped to the border.
__device__ __forceinline__ RenderTaps render_taps(float b0, float b1, float b2, const float* __restrict__ t0, const float* __restrict__ t1,
                                                  const float* __restrict__ t2, int Ht, int Wt, int flip_v) {
  const float u = b0 * t0[0] + b1 * t1[0] + b2 * t2[0];
  float v = b0 * t0[1] + b1 * t1[1] + b2 * t2[1];
  if (flip_v) v = 1.0f - v;
  // fmaxf first: a NaN becomes 0, so the taps stay inside the plane whatever the inputs hold
  const float x = fminf(fmaxf(u * (float)(Wt - 1), 0.0f), (float)(Wt - 1));
  const float y = fminf(fmaxf(v * (float)(Ht - 1), 0.0f), (float)(Ht - 1));
  const float xw = floorf(x), yn = floorf(y);
  const float w = x - xw, e = 1.0f - w, s = y - yn, nn = 1.0f - s;
  RenderTaps k;
  k.xi = (int)xw, k.yi = (int)yn;
  k.east = k.xi + 1 <= Wt - 1, k.south = k.yi + 1 <= Ht - 1;
  k.nw = nn * e, k.ne = nn * w, k.sw = s * e, k.se = s * w;
  return k;
}

// One channel: p is texel (yi, xi) of the channel's plane.  nw + ne + sw + se of the weighted taps in that order, where the ne
// product is rounded and every other product is fused into the sum (one rounding each).  That is the contraction the compiler chose
// for this expression since the first renderer; it is spelled with fmaf so that every kernel gets the same bits wherever the
// optimiser meets the products.  A tap outside the image (the east / south tap of a position on the last column / row, weight 0)
// counts 0 and is not read.
__device__ __forceinline__ float render_tap_sum(const float* __restrict__ p, int Wt, const RenderTaps& k) {
  float a = fmaf(p[0], k.nw, (k.east ? p[1] : 0.0f) * k.ne);
  a = fmaf(k.south ? p[Wt] : 0.0f, k.sw, a);
  return fmaf(k.east && k.south ? p[Wt + 1] : 0.0f, k.se, a);
}

// The pixels a face can cover: those whose centre lies in the box of its corners, clipped to the image.  floor / ceil round
// outwards, so float rounding of the box cannot lose a pixel (the edge functions decide).  False when the face is dropped: a
// corner nearer than `near` (this also keeps every NaN and every projection through z <= 0 out), zero area, or an empty box.
__device__ __forceinline__ bool render_face_box(const RenderFace& t, float near, int H, int W, int& i0, int& i1, int& j0, int& j1) {
  if (!(t.az >= near && t.bz >= near && t.cz >= near)) return false;
  if (!(fabsf(t.area) > 0.0f)) return false;
  // clamp in float first: a coordinate far outside the image must not overflow the conversion
  const float ulo = fminf(fmaxf(fminf(fminf(t.ax, t.bx), t.cx), -2.0f), (float)W + 2.0f);
  const float uhi = fminf(fmaxf(fmaxf(fmaxf(t.ax, t.bx), t.cx), -2.0f), (float)W + 2.0f);
  const float vlo = fminf(fmaxf(fminf(fminf(t.ay, t.by), t.cy), -2.0f), (float)H + 2.0f);
  const float vhi = fminf(fmaxf(fmaxf(fmaxf(t.ay, t.by), t.cy), -2.0f), (float)H + 2.0f);
  j0 = max(0, (int)floorf(ulo - 0.5f)), j1 = min(W - 1, (int)ceilf(uhi - 0.5f));
  i0 = max(0, (int)floorf(vlo - 0.5f)), i1 = min(H - 1, (int)ceilf(vhi - 0.5f));
  return j1 >= j0 && i1 >= i0;
}

// key = depth bits (positive float: ordered like the integer) << 32 | face.  The plain read first spares the atomic where a nearer
// face is already stored: the key only ever decreases, so a stale read can only cost an atomic that changes nothing.
__device__ __forceinline__ void render_cover_pixel(const RenderFace& t, int f, int i, int j, int W, unsigned long long* __restrict__ key) {
  float qa, qb, qc, depth;
  if (!render_pixel(t, i, j, qa, qb, qc, depth)) return;
  const unsigned long long mine = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned)f;
  unsigned long long* k = key + ((int64_t)i * W + j);
  if (__hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > mine) atomicMin(k, mine);
}

// Pass A.  Grid fblocks * N (fblocks = ceil(F / RENDER_THREADS); block b is face block b % fblocks of frame b / fblocks).  First
// every thread takes one face: body-mesh triangles span a few pixels, so a face with a box of at most RENDER_SMALL_BOX pixels is
// walked by its own thread (64 faces per wave in flight instead of one).  A larger face goes on the block's list in LDS, and after
// the barrier the block's waves take the listed faces in turn, 64 lanes striding over the box.  The list's order varies between
// runs; the result does not, since the minimum is taken over the same set of keys.  key [N, H, W] starts as all ones.
__global__ __launch_bounds__(RENDER_THREADS) void render_cover_kernel(
    const float* __restrict__ proj, int V, const int* __restrict__ vi, int F, int fblocks, int H, int W, float near,
    unsigned long long* __restrict__ key) {
  __shared__ int large[RENDER_THREADS];
  __shared__ int n_large;
  if (threadIdx.x == 0) n_large = 0;
  __syncthreads();
  const int64_t n = blockIdx.x / fblocks;
  const float* p = proj + n * V * 3;
  unsigned long long* kn = key + n * H * W;
  const int f = (blockIdx.x % fblocks) * RENDER_THREADS + threadIdx.x;
  int i0, i1, j0, j1;
  if (f < F) {
    const RenderFace t = render_load_face(p, vi + 3 * (int64_t)f);
    if (render_face_box(t, near, H, W, i0, i1, j0, j1)) {
      if ((int64_t)(i1 - i0 + 1) * (j1 - j0 + 1) <= RENDER_SMALL_BOX) {
        for (int i = i0; i <= i1; ++i)
          for (int j = j0; j <= j1; ++j) render_cover_pixel(t, f, i, j, W, kn);
      } else {
        large[atomicAdd(&n_large, 1)] = f;                          // an LDS integer counter: at most RENDER_THREADS entries
      }
    }
  }
  __syncthreads();
  const int lane = threadIdx.x % 64, count = n_large;
  for (int e = threadIdx.x / 64; e < count; e += RENDER_THREADS / 64) {
    const int g = large[e];
    const RenderFace t = render_load_face(p, vi + 3 * (int64_t)g);
    render_face_box(t, near, H, W, i0, i1, j0, j1);                // true: the face was listed
    const int bw = j1 - j0 + 1;
    const int64_t pixels = (int64_t)bw * (i1 - i0 + 1);
    for (int64_t q = lane; q < pixels; q += 64) render_cover_pixel(t, g, i0 + (int)(q / bw), j0 + (int)(q % bw), W, kn);
  }
}

// Pass B.  One thread per pixel and frame (grid ceil(N H W / RENDER_THREADS)): the winning face's perspective-correct barycentrics
// q / s at the centre, by the same render_pixel as the cover pass, and the depth stored in the key.  face [N, H, W] (-1), bary [N,
// H, W, 3] (0), depth [N, H, W] (0); a NULL output is skipped, every pixel of the others is written.
__global__ __launch_bounds__(RENDER_THREADS) void render_resolve_kernel(
    const float* __restrict__ proj, int V, const int* __restrict__ vi, int H, int W, int64_t total,
    const unsigned long long* __restrict__ key, int* __restrict__ face, float* __restrict__ bary, float* __restrict__ depth) {
  const int64_t t = (int64_t)blockIdx.x * RENDER_THREADS + threadIdx.x;
  if (t >= total) return;
  const unsigned long long k = key[t];
  int f = -1;
  float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, z = 0.0f;
  if (k != RENDER_EMPTY_KEY) {
    const int64_t hw = (int64_t)H * W, n = t / hw;
    const int pix = (int)(t % hw);
    f = (int)(unsigned)(k & 0xffffffffull);
    const RenderFace tri = render_load_face(proj + n * V * 3, vi + 3 * (int64_t)f);
    render_barycentrics(tri, pix / W, pix % W, b0, b1, b2);
    z = __uint_as_float((unsigned)(k >> 32));
  }
  if (face) face[t] = f;
  if (depth) depth[t] = z;
  if (bary) {
    bary[3 * t] = b0;
    bary[3 * t + 1] = b1;
    bary[3 * t + 2] = b2;
  }
}

// Pass C1.  Grid pblocks * N (pblocks = ceil(H W / RENDER_THREADS); block b is pixel block b % pblocks of frame b / pblocks).  A
// thread owns one pixel of one frame: out[n][c][pixel] = b0 x[n][i0][c] + b1 x[n][i1][c] + b2 x[n][i2][c] with (i0, i1, i2) =
// vi[face], 0 where the face is outside [0, F).  Consecutive threads write consecutive pixels of one plane, like
// surface_to_uv_kernel; unlike there the fragments belong to the frame, so a frame group would have nothing to share.
__global__ __launch_bounds__(RENDER_THREADS) void render_interpolate_kernel(
    const float* __restrict__ values, int V, int C, const int* __restrict__ vi, int F, const int* __restrict__ face,
    const float* __restrict__ bary, int64_t HW, int pblocks, float* __restrict__ out) {
  const int64_t n = blockIdx.x / pblocks;
  const int64_t pix = (int64_t)(blockIdx.x % pblocks) * RENDER_THREADS + threadIdx.x;
  if (pix >= HW) return;
  const int64_t t = n * HW + pix;
  const int f = face[t];
  float* o = out + n * C * HW + pix;
  if (f < 0 || f >= F) {
    for (int c = 0; c < C; ++c) o[c * HW] = 0.0f;
    return;
  }
  const float b0 = bary[3 * t], b1 = bary[3 * t + 1], b2 = bary[3 * t + 2];
  const float* x = values + n * V * C;
  const float* x0 = x + (int64_t)vi[3 * (int64_t)f] * C;
  const float* x1 = x + (int64_t)vi[3 * (int64_t)f + 1] * C;
  const float* x2 = x + (int64_t)vi[3 * (int64_t)f + 2] * C;
  for (int c = 0; c < C; ++c) o[c * HW] = b0 * x0[c] + b1 * x1[c] + b2 * x2[c];
}

// Pass C2.  The same grid.  The pixel's uv from the corners (t0, t1, t2) = vti[face] of vt, sampled bilinearly on tex [., C, Ht, Wt]
// as given: render_taps and render_tap_sum above.  out [N, C, H, W], 0 where the face is outside [0, F).
__global__ __launch_bounds__(RENDER_THREADS) void render_texture_kernel(
    const int* __restrict__ face, const float* __restrict__ bary, int64_t HW, int pblocks, const float* __restrict__ vt,
    const int* __restrict__ vti, int F, const float* __restrict__ tex, int64_t tex_stride, int C, int Ht, int Wt, int flip_v,
    float* __restrict__ out) {
  const int64_t n = blockIdx.x / pblocks;
  const int64_t pix = (int64_t)(blockIdx.x % pblocks) * RENDER_THREADS + threadIdx.x;
  if (pix >= HW) return;
  const int64_t t = n * HW + pix;
  const int f = face[t];
  float* o = out + n * C * HW + pix;
  if (f < 0 || f >= F) {
    for (int c = 0; c < C; ++c) o[c * HW] = 0.0f;
    return;
  }
  const float b0 = bary[3 * t], b1 = bary[3 * t + 1], b2 = bary[3 * t + 2];
  const float* t0 = vt + 2 * (int64_t)vti[3 * (int64_t)f];
  const float* t1 = vt + 2 * (int64_t)vti[3 * (int64_t)f + 1];
  const float* t2 = vt + 2 * (int64_t)vti[3 * (int64_t)f + 2];
  const RenderTaps k = render_taps(b0, b1, b2, t0, t1, t2, Ht, Wt, flip_v);
  const int64_t plane = (int64_t)Ht * Wt;
  const float* img = tex + n * tex_stride + (int64_t)k.yi * Wt + k.xi;
  for (int c = 0; c < C; ++c) o[c * HW] = render_tap_sum(img + c * plane, Wt, k);
}
