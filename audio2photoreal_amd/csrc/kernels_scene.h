// Several bodies in one image (audio2photoreal_amd/scene.py; INTEGRATION.md "Two people in one scene").  A scene is P <= SCENE_MAX_BODIES
// meshes, each with its own vertices, topology, texture and optional rigid placement.  They are projected into ONE proj [N, sum V, 3]
// and rasterised as one mesh through the merged face table [sum F, 3] (built once on the host, each body's vertex offset added): the
// key fill and render_cover_kernel of kernels_render.h run unchanged, so the z-buffer is shared per sample.  The key is still depth
// bits << 32 | global face index: at exactly equal depth the earlier body wins, then the lower face.  The resolve below is
// render_aa_kernel<true> (kernels_render_aa.h) with the face's body looked up per sample.  Per-body pointers and sizes travel by value
// in the kernel arguments (SceneDesc): nothing is uploaded per call.
#pragma once
#include "kernels_render_aa.h"

#define SCENE_MAX_BODIES 4

struct SceneBody {
  const float* verts;    // [N, V, 3]
  const float* place;    // [N or 1, 3, 4] x_world = R x + t; NULL: the vertices are world coordinates already
  const float* tex;      // [N or 1, C, Ht, Wt]
  const float* vt;       // [T, 2]
  const int* vti;        // [F, 3], the body's own face numbering
  int64_t place_stride;  // floats between the frames of place (0: shared)
  int64_t tex_stride;    // floats between the frames of tex (0: shared)
  int V, v0;             // vertices, and the body's first vertex in proj
  int f0;                // the body's first face in the merged table
  int Ht, Wt, flip_v;
};

struct SceneDesc {
  SceneBody body[SCENE_MAX_BODIES];   // entries P.. are copies of the last body with v0 = f0 = INT_MAX: never selected
  int P, V, F;                        // bodies, sum V, sum F
};

// The body of global index i among the starts s1..s3 of bodies 1..3 (INT_MAX where there is no such body): a compare chain.
__device__ __forceinline__ int scene_body_of(int i, int s1, int s2, int s3) { return (i >= s1) + (i >= s2) + (i >= s3); }

// Pass 0 for all bodies in one launch.  Grid tiles * N (tiles = ceil(sum V / RENDER_THREADS)): one thread per merged vertex and
// frame, through K' = K with its first two rows times `scale` (render_project_scaled_kernel's rule).  A body without a placement goes
// through render_project_vertex itself.  A placed body's vertex is first moved, per coordinate r, by
//   w_r = ((M[r][0] x + M[r][1] y) + M[r][2] z) + M[r][3]      in float32, every product and sum rounded (no fused multiply-add),
// and w then takes the place of the vertex in the same projection.
__global__ __launch_bounds__(RENDER_THREADS) void scene_project_kernel(SceneDesc d, int tiles, const float* __restrict__ K, int64_t k_stride,
                                                                      const float* __restrict__ Rt, int64_t rt_stride, float scale,
                                                                      float* __restrict__ proj) {
  const int64_t n = blockIdx.x / tiles;
  const int v = (blockIdx.x % tiles) * RENDER_THREADS + threadIdx.x;
  if (v >= d.V) return;
  const int p = scene_body_of(v, d.body[1].v0, d.body[2].v0, d.body[3].v0);
  SceneBody b = d.body[0];
#pragma unroll
  for (int q = 1; q < SCENE_MAX_BODIES; ++q)
    if (p == q) b = d.body[q];                                      // constant indices: selects, no table in scratch
  const float* k = K + n * k_stride;
  const float* m = Rt + n * rt_stride;
  const float k0 = k[0] * scale, k1 = k[1] * scale, k2 = k[2] * scale, k4 = k[4] * scale, k5 = k[5] * scale;
  const int64_t in = 3 * (n * b.V + (v - b.v0));                    // the vertex in the body's own array
  if (!b.place) {
    // proj + 3 (n (sum V - V_p) + v0_p) + in is the vertex's place in the merged array; the shifted base lies inside proj
    render_project_vertex(b.verts, m, k0, k1, k2, k4, k5, in, proj + 3 * (n * (d.V - b.V) + b.v0));
    return;
  }
  const float* M = b.place + n * b.place_stride;
  const float x = b.verts[in], y = b.verts[in + 1], z = b.verts[in + 2];
  float w[3];                                                       // constant indices after inlining: registers
  {
#pragma clang fp contract(off)
    w[0] = M[0] * x + M[1] * y + M[2] * z + M[3];
    w[1] = M[4] * x + M[5] * y + M[6] * z + M[7];
    w[2] = M[8] * x + M[9] * y + M[10] * z + M[11];
  }
  render_project_vertex(w, m, k0, k1, k2, k4, k5, 0, proj + 3 * (n * d.V + v));
}

// Resolve + shade + downsample for a scene: render_aa_kernel<true> with the sample's body found from its global face index.  Grid
// pblocks * N, a thread per output pixel and frame; samples walked a outer, b inner; the face's corners, uv corners and the body's
// texture are kept while consecutive samples hold the same face.  Shading is render_texture_kernel's bilinear expression on the
// body's own vt / vti / texture / flip.  fp32 accumulators from 0: alpha = n / S^2, mean = acc / S^2, depth = sum of the samples'
// depths / S^2 (an uncovered sample counts 0), body_alpha[p] = n_p / S^2 with n_p the samples body p wins (sum over p = n).
// n == S^2 -> mean (bg not read), n == 0 -> bg, else mean + (1 - alpha) bg; without bg, mean.  Accumulators and the per-body
// counters are indexed by unrolled constants only: registers, no scratch.
__global__ __launch_bounds__(RENDER_THREADS) void scene_resolve_kernel(
    SceneDesc d, const float* __restrict__ proj, const int* __restrict__ vi, const unsigned long long* __restrict__ key, int H, int W, int S,
    int pblocks, int C, const float* __restrict__ bg, int64_t bg_stride, float* __restrict__ out, float* __restrict__ alpha,
    float* __restrict__ depth, float* __restrict__ body_alpha) {
  const int64_t n = blockIdx.x / pblocks;
  const int64_t HW = (int64_t)H * W;
  const int64_t pix = (int64_t)(blockIdx.x % pblocks) * RENDER_THREADS + threadIdx.x;
  if (pix >= HW) return;
  const int i = (int)(pix / W), j = (int)(pix % W);
  const int64_t sW = (int64_t)S * W;
  const unsigned long long* kn = key + n * HW * S * S;
  const float* p = proj + n * d.V * 3;
  float acc[RENDER_MAX_CHANNELS];
#pragma unroll
  for (int c = 0; c < RENDER_MAX_CHANNELS; ++c) acc[c] = 0.0f;
  int cnt[SCENE_MAX_BODIES];
#pragma unroll
  for (int q = 0; q < SCENE_MAX_BODIES; ++q) cnt[q] = 0;
  float zacc = 0.0f;
  int count = 0, held = -1, body = 0;
  RenderFace tri = {};
  const float *c0 = nullptr, *c1 = nullptr, *c2 = nullptr;           // uv corners of the held face
  const float* data = nullptr;                                       // the held face's texture, this frame
  int Ht = 1, Wt = 1, flip_v = 0;
  for (int a = 0; a < S; ++a) {
    const int si = S * i + a;
    const unsigned long long* krow = kn + si * sW + (int64_t)S * j;
    for (int b = 0; b < S; ++b) {
      const unsigned long long k = krow[b];
      if (k == RENDER_EMPTY_KEY) continue;
      const int f = (int)(unsigned)(k & 0xffffffffull);
      if (f != held) {
        held = f;
        tri = render_load_face(p, vi + 3 * (int64_t)f);
        body = scene_body_of(f, d.body[1].f0, d.body[2].f0, d.body[3].f0);
        const float* vt = d.body[0].vt;
        const int* tab = d.body[0].vti;
        int f0 = 0;
        data = d.body[0].tex + n * d.body[0].tex_stride;
        Ht = d.body[0].Ht, Wt = d.body[0].Wt, flip_v = d.body[0].flip_v;
#pragma unroll
        for (int q = 1; q < SCENE_MAX_BODIES; ++q) {
          if (body == q) {
            vt = d.body[q].vt, tab = d.body[q].vti, f0 = d.body[q].f0;
            data = d.body[q].tex + n * d.body[q].tex_stride;
            Ht = d.body[q].Ht, Wt = d.body[q].Wt, flip_v = d.body[q].flip_v;
          }
        }
        const int* t = tab + 3 * (int64_t)(f - f0);
        c0 = vt + t[0] * 2, c1 = vt + t[1] * 2, c2 = vt + t[2] * 2;
      }
      float qa, qb, qc, dd;
      render_pixel(tri, si, S * j + b, qa, qb, qc, dd);
      const float s = qa + qb + qc;
      const float b0 = qa / s, b1 = qb / s, b2 = qc / s;
      ++count;
#pragma unroll
      for (int q = 0; q < SCENE_MAX_BODIES; ++q) cnt[q] += body == q;
      zacc += __uint_as_float((unsigned)(k >> 32));
      const float u = b0 * c0[0] + b1 * c1[0] + b2 * c2[0];
      float v = b0 * c0[1] + b1 * c1[1] + b2 * c2[1];
      if (flip_v) v = 1.0f - v;
      // fmaxf first: a NaN becomes 0, so the taps stay inside the plane whatever the inputs hold
      const float x = fminf(fmaxf(u * (float)(Wt - 1), 0.0f), (float)(Wt - 1));
      const float y = fminf(fmaxf(v * (float)(Ht - 1), 0.0f), (float)(Ht - 1));
      const float xw = floorf(x), yn = floorf(y);
      const float we = x - xw, e = 1.0f - we, so = y - yn, nn = 1.0f - so;
      const int xi = (int)xw, yi = (int)yn;
      const bool east = xi + 1 <= Wt - 1, south = yi + 1 <= Ht - 1;
      const int64_t plane = (int64_t)Ht * Wt;
      const float* img = data + (int64_t)yi * Wt + xi;
#pragma unroll
      for (int c = 0; c < RENDER_MAX_CHANNELS; ++c) {
        if (c < C) {
          const float* t = img + c * plane;
          float r = t[0] * (nn * e);
          r += (east ? t[1] : 0.0f) * (nn * we);
          r += (south ? t[Wt] : 0.0f) * (so * e);
          r += (east && south ? t[Wt + 1] : 0.0f) * (so * we);
          acc[c] += r;
        }
      }
    }
  }
  {
#pragma clang fp contract(off)      // the resolve as stated: divisions, then a product and a sum, each rounded
    const float ss = (float)(S * S);
    const float cover = (float)count / ss;
    const bool full = count == S * S, none = count == 0;
    alpha[n * HW + pix] = cover;
    depth[n * HW + pix] = zacc / ss;
    float* ba = body_alpha + n * d.P * HW + pix;
#pragma unroll
    for (int q = 0; q < SCENE_MAX_BODIES; ++q)
      if (q < d.P) ba[q * HW] = (float)cnt[q] / ss;
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
