// Anti-aliased rendered images (audio2photoreal_amd/render.py render_antialiased / interpolate_antialiased; INTEGRATION.md "Rendered
// images", the supersampling rule).  S samples per axis: sample (a, b) of pixel (i, j) is pixel (S i + a, S j + b) of the S H x S W
// image seen through K' = K with its first two rows times S in float32.  Projection (scale S), key fill and cover pass run unchanged
// on that grid (kernels_render.h); the one pass here reads the [N, S H, S W] keys and writes only the [N, C, H, W] image, its coverage
// and its depth.  What a sample is shaded from is a source type: hold(f) takes up face f when the walk reaches another face,
// sample(b0, b1, b2) one sample's barycentrics, channel(c) gives that sample's value in channel c.  All members are inlined and the
// type is a template argument: no kernel branches on the kind of source.
#pragma once
#include "kernels_render.h"

// The kernel argument of render_aa_kernel: a UV texture (TEX) or per-vertex values.  tab is vti [F, 3] for a texture, vi for values.
struct RenderAASource {
  const float* data;     // tex [N or 1, C, Ht, Wt] | values [N, V, C]
  int64_t stride;        // floats between the frames of data (0: shared)
  const float* vt;       // [T, 2]; texture only
  const int* tab;
  int Ht, Wt, flip_v;    // texture only
};

// Per-vertex values: render_interpolate_kernel's expression on the value rows of the held face's corners.
struct RenderValueSource {
  const float* rows;     // values [V, C] of this frame
  const int* tab;
  int64_t C;
  const float *c0 = nullptr, *c1 = nullptr, *c2 = nullptr;
  float b0, b1, b2;
  __device__ __forceinline__ RenderValueSource(const RenderAASource& s, int64_t n, int C) : rows(s.data + n * s.stride), tab(s.tab), C(C) {}
  __device__ __forceinline__ void hold(int f) {
    const int* t = tab + 3 * (int64_t)f;
    c0 = rows + t[0] * C, c1 = rows + t[1] * C, c2 = rows + t[2] * C;
  }
  __device__ __forceinline__ void sample(float a0, float a1, float a2) { b0 = a0, b1 = a1, b2 = a2; }
  __device__ __forceinline__ float channel(int c) const { return b0 * c0[c] + b1 * c1[c] + b2 * c2[c]; }
};

// One body's UV texture: render_texture_kernel's bilinear expression on the uv corners of the held face.
struct RenderTextureSource {
  const float* data = nullptr;   // tex [C, Ht, Wt] of this frame
  const float* vt = nullptr;
  const int* tab = nullptr;
  int Ht = 1, Wt = 1, flip_v = 0;
  const float *c0 = nullptr, *c1 = nullptr, *c2 = nullptr;
  RenderTaps k;
  const float* img;              // texel (yi, xi) of channel 0
  RenderTextureSource() = default;
  __device__ __forceinline__ RenderTextureSource(const RenderAASource& s, int64_t n, int)
      : data(s.data + n * s.stride), vt(s.vt), tab(s.tab), Ht(s.Ht), Wt(s.Wt), flip_v(s.flip_v) {}
  __device__ __forceinline__ void hold(int f) {
    const int* t = tab + 3 * (int64_t)f;
    c0 = vt + t[0] * (int64_t)2, c1 = vt + t[1] * (int64_t)2, c2 = vt + t[2] * (int64_t)2;
  }
  __device__ __forceinline__ void sample(float b0, float b1, float b2) {
    k = render_taps(b0, b1, b2, c0, c1, c2, Ht, Wt, flip_v);
    img = data + (int64_t)k.yi * Wt + k.xi;
  }
  __device__ __forceinline__ float channel(int c) const { return render_tap_sum(img + c * ((int64_t)Ht * Wt), Wt, k); }
};

// Resolve + shade + downsample of output pixel pix of frame n; p, key: the frame's proj and [S H, S W] keys.  The samples are walked
// a outer, b inner; a sample's barycentrics are render_barycentrics at (S i + a, S j + b), as render_resolve_kernel computes them.
// The face's corners (and what hold() keeps) stay while consecutive samples hold the same face (most of a pixel's samples do).  fp32
// accumulators from 0; alpha = n / S^2, mean = acc / S^2, depth = sum of the samples' depths / S^2 (divisions; an uncovered sample
// counts 0); n == S^2 -> mean (bg not read), n == 0 -> bg, else mean + (1 - alpha) bg; without bg, mean.  alpha, depth (NULL: not
// written) [N, 1, H, W], out [N, C, H, W].  Accumulators are indexed by unrolled constants only: registers, no scratch.
template <class Source>
__device__ __forceinline__ void render_aa_pixel(Source& src, const float* __restrict__ p, const int* __restrict__ vi,
                                                const unsigned long long* __restrict__ key, int H, int W, int S, int64_t n, int64_t pix, int C,
                                                const float* __restrict__ bg, int64_t bg_stride, float* __restrict__ out,
                                                float* __restrict__ alpha, float* __restrict__ depth) {
  const int64_t HW = (int64_t)H * W;
  const int i = (int)(pix / W), j = (int)(pix % W);
  const int64_t sW = (int64_t)S * W;
  float acc[RENDER_MAX_CHANNELS];
#pragma unroll
  for (int c = 0; c < RENDER_MAX_CHANNELS; ++c) acc[c] = 0.0f;
  float zacc = 0.0f;
  int count = 0, held = -1;
  RenderFace tri = {};
  for (int a = 0; a < S; ++a) {
    const int si = S * i + a;
    const unsigned long long* krow = key + si * sW + (int64_t)S * j;
    for (int b = 0; b < S; ++b) {
      const unsigned long long k = krow[b];
      if (k == RENDER_EMPTY_KEY) continue;
      const int f = (int)(unsigned)(k & 0xffffffffull);
      if (f != held) {
        held = f;
        tri = render_load_face(p, vi + 3 * (int64_t)f);
        src.hold(f);
      }
      float b0, b1, b2;
      render_barycentrics(tri, si, S * j + b, b0, b1, b2);
      ++count;
      zacc += __uint_as_float((unsigned)(k >> 32));
      src.sample(b0, b1, b2);
#pragma unroll
      for (int c = 0; c < RENDER_MAX_CHANNELS; ++c)
        if (c < C) acc[c] += src.channel(c);
    }
  }
  {
#pragma clang fp contract(off)      // the resolve as stated: two divisions, then a product and a sum, each rounded
    const float ss = (float)(S * S);
    const float cover = (float)count / ss;
    const bool full = count == S * S, none = count == 0;
    alpha[n * HW + pix] = cover;
    if (depth) depth[n * HW + pix] = zacc / ss;
    float* o = out + n * C * HW + pix;
    const float* g = bg ? bg + n * bg_stride + pix : nullptr;
#pragma unroll
    for (int c = 0; c < RENDER_MAX_CHANNELS; ++c) {
      if (c < C) {
        float r = acc[c] / ss;
        if (g && !full) {
          const float back = g[c * HW];
          r = none ? back : r + (1.0f - cover) * back;
        }
        o[c * HW] = r;
      }
    }
  }
}

// Grid pblocks * N (pblocks = ceil(H W / RENDER_THREADS)): a thread owns one output pixel of one frame, consecutive lanes consecutive
// pixels of a plane, so the C + 1 (+ 1) plane stores are coalesced and a wave reads 64 S contiguous keys of a sample row.
template <bool TEX>
__global__ __launch_bounds__(RENDER_THREADS) void render_aa_kernel(
    const float* __restrict__ proj, int V, const int* __restrict__ vi, const unsigned long long* __restrict__ key, int H, int W, int S,
    int pblocks, RenderAASource src, int C, const float* __restrict__ bg, int64_t bg_stride, float* __restrict__ out,
    float* __restrict__ alpha, float* __restrict__ depth) {
  const int64_t n = blockIdx.x / pblocks, HW = (int64_t)H * W;
  const int64_t pix = (int64_t)(blockIdx.x % pblocks) * RENDER_THREADS + threadIdx.x;
  if (pix >= HW) return;
  typename std::conditional<TEX, RenderTextureSource, RenderValueSource>::type source(src, n, C);
  render_aa_pixel(source, proj + n * V * 3, vi, key + n * HW * S * S, H, W, S, n, pix, C, bg, bg_stride, out, alpha, depth);
}
