// Several bodies in one image (audio2photoreal_amd/scene.py; INTEGRATION.md "Two people in one scene").  A scene is P <= SCENE_MAX_BODIES
// meshes, each with its own vertices, topology, texture and optional rigid placement.  They are projected into ONE proj [N, sum V, 3]
// and rasterised as one mesh through the merged face table [sum F, 3] (built once on the host, each body's vertex offset added): the
// key fill and render_cover_kernel of kernels_render.h run unchanged, so the z-buffer is shared per sample.  The key is still depth
// bits << 32 | global face index: at exactly equal depth the earlier body wins, then the lower face.  The resolve below is
// render_aa_pixel (kernels_render_aa.h) over a source that looks the face's body up where the face changes.  Per-body pointers and sizes travel by value
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

// The textures of a scene's bodies as one source: the held face's body is found from its global face index, that body's vt / vti /
// texture / flip shade the sample (RenderTextureSource), and the samples each body wins are counted.  The body's fields are chosen
// by a select chain over d.body[q] with constant q and the counters indexed by unrolled constants only: registers, no scratch.
struct SceneSource {
  const SceneDesc& d;
  int64_t n;
  RenderTextureSource cur;            // the held face's body, this frame
  int body = 0, f0 = 0;
  int cnt[SCENE_MAX_BODIES] = {};
  __device__ __forceinline__ SceneSource(const SceneDesc& d, int64_t n) : d(d), n(n) {}
  __device__ __forceinline__ void take(const SceneBody& b) {
    cur.vt = b.vt, cur.tab = b.vti, f0 = b.f0;
    cur.data = b.tex + n * b.tex_stride;
    cur.Ht = b.Ht, cur.Wt = b.Wt, cur.flip_v = b.flip_v;
  }
  __device__ __forceinline__ void hold(int f) {
    body = scene_body_of(f, d.body[1].f0, d.body[2].f0, d.body[3].f0);
    take(d.body[0]);
#pragma unroll
    for (int q = 1; q < SCENE_MAX_BODIES; ++q)
      if (body == q) take(d.body[q]);
    cur.hold(f - f0);
  }
  __device__ __forceinline__ void sample(float b0, float b1, float b2) {
#pragma unroll
    for (int q = 0; q < SCENE_MAX_BODIES; ++q) cnt[q] += body == q;
    cur.sample(b0, b1, b2);
  }
  __device__ __forceinline__ float channel(int c) const { return cur.channel(c); }
};

// Resolve + shade + downsample for a scene: render_aa_pixel (kernels_render_aa.h) over a SceneSource, on render_aa_kernel's grid,
// and body_alpha[p] = n_p / S^2 with n_p the samples body p wins (their sum over p is alpha S^2).
__global__ __launch_bounds__(RENDER_THREADS) void scene_resolve_kernel(
    SceneDesc d, const float* __restrict__ proj, const int* __restrict__ vi, const unsigned long long* __restrict__ key, int H, int W, int S,
    int pblocks, int C, const float* __restrict__ bg, int64_t bg_stride, float* __restrict__ out, float* __restrict__ alpha,
    float* __restrict__ depth, float* __restrict__ body_alpha) {
  const int64_t n = blockIdx.x / pblocks, HW = (int64_t)H * W;
  const int64_t pix = (int64_t)(blockIdx.x % pblocks) * RENDER_THREADS + threadIdx.x;
  if (pix >= HW) return;
  SceneSource source(d, n);
  render_aa_pixel(source, proj + n * d.V * 3, vi, key + n * HW * S * S, H, W, S, n, pix, C, bg, bg_stride, out, alpha, depth);
  {
#pragma clang fp contract(off)      // part of the resolve: a division like alpha's
    float* ba = body_alpha + n * d.P * HW + pix;
#pragma unroll
    for (int q = 0; q < SCENE_MAX_BODIES; ++q)
      if (q < d.P) ba[q * HW] = (float)source.cnt[q] / (float)(S * S);
  }
}
