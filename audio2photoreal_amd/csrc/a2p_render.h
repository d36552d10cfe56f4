// C ABI of the rendered images (include/a2p_hip.h "rendered images"; kernels in kernels_render.h).  Context-free like the surface
// maps: the topology tables are device arrays the caller built once (audio2photoreal_amd/surface.py validates them on the host).
// Included at the end of a2p_lib.hip (set_err / ARG / HIPCHK).
#pragma once

static inline int64_t render_tiles(int64_t n) { return (n + RENDER_THREADS - 1) / RENDER_THREADS; }

extern "C" int a2p_render_rasterize(const float* verts, int64_t N, int32_t V, const int32_t* vi, int32_t F, const float* K,
                                    int32_t k_per_frame, const float* Rt, int32_t rt_per_frame, int32_t H, int32_t W, float near,
                                    float* proj, uint64_t* key, int32_t* face, float* bary, float* depth, void* stream) {
  static_assert(RENDER_MAX_SIZE == A2P_RENDER_MAX_SIZE && RENDER_MAX_CHANNELS == A2P_RENDER_MAX_CHANNELS, "render limits");
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the key is one 64-bit word");
  ARG(verts && vi && K && Rt && proj && key, "render_rasterize: null argument");
  ARG(face || bary || depth, "render_rasterize: all three outputs are null");
  ARG(V >= 1 && F >= 1 && (int64_t)F * 3 <= 0x7fffffff, "render_rasterize: V=%d, F=%d: need V >= 1, 1 <= 3 F < 2^31", V, F);
  ARG(H >= 1 && H <= A2P_RENDER_MAX_SIZE && W >= 1 && W <= A2P_RENDER_MAX_SIZE, "render_rasterize: a %d x %d image: need 1 <= H, W <= %d",
      H, W, A2P_RENDER_MAX_SIZE);
  ARG(near > 0.0f && near < __builtin_inff(), "render_rasterize: near=%g: need a positive finite distance", (double)near);
  const int64_t vtiles = render_tiles(V), fblocks = render_tiles(F), HW = (int64_t)H * W;
  ARG(N >= 0 && N <= 0x7fffffff && N * vtiles <= 0x7fffffff && N * fblocks <= 0x7fffffff,
      "render_rasterize: N=%lld frames x %lld vertex tiles or %lld face blocks exceed the grid", (long long)N, (long long)vtiles,
      (long long)fblocks);
  ARG(render_tiles(N * HW) <= 0x7fffffff, "render_rasterize: N=%lld frames of %d x %d pixels exceed the grid", (long long)N, H, W);
  const void* ins[] = {verts, vi, K, Rt};
  const void* outs[] = {proj, key, face, bary, depth};
  for (int a = 0; a < 5; ++a) {
    for (int b = 0; b < 4; ++b) ARG(outs[a] != ins[b], "render_rasterize: a scratch or output array must not alias an input");
    for (int b = 0; b < a; ++b) ARG(!outs[a] || outs[a] != outs[b], "render_rasterize: the scratch and output arrays must be distinct");
  }
  if (N == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  render_project_kernel<<<(unsigned)(N * vtiles), RENDER_THREADS, 0, s>>>(verts, V, (int)vtiles, K, k_per_frame ? 9 : 0, Rt,
                                                                          rt_per_frame ? 12 : 0, proj);
  HIPCHK(hipMemsetAsync(key, 0xff, (size_t)(N * HW) * sizeof(uint64_t), s));
  render_cover_kernel<<<(unsigned)(N * fblocks), RENDER_THREADS, 0, s>>>(proj, V, vi, F, (int)fblocks, H, W, near,
                                                                         (unsigned long long*)key);
  render_resolve_kernel<<<(unsigned)render_tiles(N * HW), RENDER_THREADS, 0, s>>>(proj, V, vi, H, W, N * HW,
                                                                                 (const unsigned long long*)key, face, bary, depth);
  HIPCHK(hipGetLastError());
  return 0;
}

// the checks the two per-pixel passes share; pblocks = pixel blocks of one frame
static int render_pixel_grid(const char* who, int64_t N, int32_t C, int32_t H, int32_t W, int64_t* pblocks) {
  ARG(C >= 1 && C <= A2P_RENDER_MAX_CHANNELS, "%s: C=%d outside [1, %d]", who, C, A2P_RENDER_MAX_CHANNELS);
  ARG(H >= 1 && H <= A2P_RENDER_MAX_SIZE && W >= 1 && W <= A2P_RENDER_MAX_SIZE, "%s: a %d x %d image: need 1 <= H, W <= %d", who, H, W,
      A2P_RENDER_MAX_SIZE);
  *pblocks = render_tiles((int64_t)H * W);
  ARG(N >= 0 && N <= 0x7fffffff && N * *pblocks <= 0x7fffffff, "%s: N=%lld frames x %lld pixel blocks exceed the grid", who, (long long)N,
      (long long)*pblocks);
  return 0;
}

extern "C" int a2p_render_interpolate(const float* values, int64_t N, int32_t V, int32_t C, const int32_t* vi, int32_t F,
                                      const int32_t* face, const float* bary, int32_t H, int32_t W, float* out, void* stream) {
  ARG(values && vi && face && bary && out, "render_interpolate: null argument");
  ARG(V >= 1 && F >= 1 && (int64_t)F * 3 <= 0x7fffffff, "render_interpolate: V=%d, F=%d: need V >= 1, 1 <= 3 F < 2^31", V, F);
  int64_t pblocks;
  CHK(render_pixel_grid("render_interpolate", N, C, H, W, &pblocks));
  ARG(out != values && (const float*)out != bary && (const void*)out != (const void*)face && (const void*)out != (const void*)vi,
      "render_interpolate: out must not alias an input");
  if (N == 0) return 0;
  render_interpolate_kernel<<<(unsigned)(N * pblocks), RENDER_THREADS, 0, (hipStream_t)stream>>>(values, V, C, vi, F, face, bary,
                                                                                                (int64_t)H * W, (int)pblocks, out);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_render_texture(const int32_t* face, const float* bary, int64_t N, int32_t H, int32_t W, const float* vt, int32_t T,
                                  const int32_t* vti, int32_t F, const float* tex, int32_t tex_per_frame, int32_t C, int32_t Ht,
                                  int32_t Wt, int32_t flip_v, float* out, void* stream) {
  ARG(face && bary && vt && vti && tex && out, "render_texture: null argument");
  ARG(T >= 1 && F >= 1 && (int64_t)F * 3 <= 0x7fffffff, "render_texture: T=%d, F=%d: need T >= 1, 1 <= 3 F < 2^31", T, F);
  ARG(Ht >= 1 && Wt >= 1 && (int64_t)Ht * Wt <= 0x7fffffff, "render_texture: a %d x %d texture: need 1 <= Ht Wt < 2^31", Ht, Wt);
  int64_t pblocks;
  CHK(render_pixel_grid("render_texture", N, C, H, W, &pblocks));
  ARG(out != tex && (const float*)out != bary && (const float*)out != vt && (const void*)out != (const void*)face &&
          (const void*)out != (const void*)vti,
      "render_texture: out must not alias an input");
  if (N == 0) return 0;
  render_texture_kernel<<<(unsigned)(N * pblocks), RENDER_THREADS, 0, (hipStream_t)stream>>>(
      face, bary, (int64_t)H * W, (int)pblocks, vt, vti, F, tex, tex_per_frame ? (int64_t)C * Ht * Wt : 0, C, Ht, Wt, flip_v, out);
  HIPCHK(hipGetLastError());
  return 0;
}
