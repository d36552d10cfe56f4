// C ABI of the rendered images (include/a2p_hip.h "rendered images"; kernels in kernels_render.h).  Context-free like the surface
// maps: the topology tables are device arrays the caller built once (audio2photoreal_amd/surface.py validates them on the host).
// Included at the end of a2p_lib.hip (set_err / ARG / HIPCHK).
#pragma once

static inline int64_t render_tiles(int64_t n) { return (n + RENDER_THREADS - 1) / RENDER_THREADS; }

// ---- what the rasterising entry points (three here, one in a2p_scene.h) share; `who` names the caller in every message
static int render_samples(const char* who, int32_t H, int32_t W, int32_t S, float near) {
  ARG(S >= 1 && S <= A2P_RENDER_MAX_SUPERSAMPLE, "%s: S=%d samples per axis: need 1 <= S <= %d", who, S, A2P_RENDER_MAX_SUPERSAMPLE);
  ARG(H >= 1 && W >= 1 && (int64_t)S * H <= A2P_RENDER_MAX_SIZE && (int64_t)S * W <= A2P_RENDER_MAX_SIZE,
      "%s: a %d x %d image at S=%d: need 1 <= H, W and S H, S W <= %d", who, H, W, S, A2P_RENDER_MAX_SIZE);
  ARG(near > 0.0f && near < __builtin_inff(), "%s: near=%g: need a positive finite distance", who, (double)near);
  return 0;
}

static int render_mesh_grid(const char* who, int64_t N, int64_t V, int64_t F) {      // the grids of the projection and the cover pass
  ARG(N >= 0 && N <= 0x7fffffff && N * render_tiles(V) <= 0x7fffffff && N * render_tiles(F) <= 0x7fffffff,
      "%s: N=%lld frames x %lld vertex tiles or %lld face blocks exceed the grid", who, (long long)N, (long long)render_tiles(V),
      (long long)render_tiles(F));
  return 0;
}

// no scratch or output array is an input or another of them; a null entry on either side is an array that is not there
static int render_distinct(const char* who, std::initializer_list<const void*> outs, std::initializer_list<const void*> ins) {
  for (const void* const* a = outs.begin(); a != outs.end(); ++a) {
    for (const void* b : ins) ARG(!*a || *a != b, "%s: a scratch or output array must not alias an input", who);
    for (const void* const* b = outs.begin(); b != a; ++b) ARG(!*a || *a != *b, "%s: the scratch and output arrays must be distinct", who);
  }
  return 0;
}

// Passes 0 and A on the S H x S W sample grid (kernels_render.h): the projection of one mesh, or of a scene's bodies when `scene` is
// given, into proj [N, V, 3] through K with its first two rows times S; the key fill; the cover pass over faces [F, 3].
static int render_front(const SceneDesc* scene, const float* verts, int32_t V, const int32_t* faces, int32_t F, int64_t N, const float* K,
                        int32_t k_per_frame, const float* Rt, int32_t rt_per_frame, int32_t H, int32_t W, int32_t S, float near,
                        float* proj, uint64_t* key, hipStream_t s) {
  const int64_t vtiles = render_tiles(V), fblocks = render_tiles(F), ks = k_per_frame ? 9 : 0, rs = rt_per_frame ? 12 : 0;
  const unsigned grid = (unsigned)(N * vtiles);
  if (scene) scene_project_kernel<<<grid, RENDER_THREADS, 0, s>>>(*scene, (int)vtiles, K, ks, Rt, rs, (float)S, proj);
  else render_project_scaled_kernel<<<grid, RENDER_THREADS, 0, s>>>(verts, V, (int)vtiles, K, ks, Rt, rs, (float)S, proj);
  HIPCHK(hipMemsetAsync(key, 0xff, (size_t)(N * S * H * S * W) * sizeof(uint64_t), s));
  render_cover_kernel<<<(unsigned)(N * fblocks), RENDER_THREADS, 0, s>>>(proj, V, faces, F, (int)fblocks, S * H, S * W, near,
                                                                         (unsigned long long*)key);
  return 0;
}

extern "C" int a2p_render_rasterize(const float* verts, int64_t N, int32_t V, const int32_t* vi, int32_t F, const float* K,
                                    int32_t k_per_frame, const float* Rt, int32_t rt_per_frame, int32_t H, int32_t W, float near,
                                    float* proj, uint64_t* key, int32_t* face, float* bary, float* depth, void* stream) {
  static_assert(RENDER_MAX_SIZE == A2P_RENDER_MAX_SIZE && RENDER_MAX_CHANNELS == A2P_RENDER_MAX_CHANNELS, "render limits");
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the key is one 64-bit word");
  const char* who = "render_rasterize";
  ARG(verts && vi && K && Rt && proj && key, "%s: null argument", who);
  ARG(face || bary || depth, "%s: all three outputs are null", who);
  ARG(V >= 1 && F >= 1 && (int64_t)F * 3 <= 0x7fffffff, "%s: V=%d, F=%d: need V >= 1, 1 <= 3 F < 2^31", who, V, F);
  ARG(H >= 1 && H <= A2P_RENDER_MAX_SIZE && W >= 1 && W <= A2P_RENDER_MAX_SIZE, "%s: a %d x %d image: need 1 <= H, W <= %d", who, H, W,
      A2P_RENDER_MAX_SIZE);
  CHK(render_samples(who, H, W, 1, near));                           // one sample per pixel: only `near` is left to refuse
  CHK(render_mesh_grid(who, N, V, F));
  const int64_t HW = (int64_t)H * W;
  ARG(render_tiles(N * HW) <= 0x7fffffff, "%s: N=%lld frames of %d x %d pixels exceed the grid", who, (long long)N, H, W);
  CHK(render_distinct(who, {proj, key, face, bary, depth}, {verts, vi, K, Rt}));
  if (N == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  CHK(render_front(nullptr, verts, V, vi, F, N, K, k_per_frame, Rt, rt_per_frame, H, W, 1, near, proj, key, s));   // scale 1: K itself
  render_resolve_kernel<<<(unsigned)render_tiles(N * HW), RENDER_THREADS, 0, s>>>(proj, V, vi, H, W, N * HW,
                                                                                 (const unsigned long long*)key, face, bary, depth);
  HIPCHK(hipGetLastError());
  return 0;
}

// the checks the per-pixel passes share; pblocks = pixel blocks of one frame
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

// ---- anti-aliased images (kernels_render_aa.h): project, key fill, cover on the S H x S W grid and the fused resolve, in one call
static int render_aa_run(const char* who, const float* verts, int64_t N, int32_t V, const int32_t* vi, int32_t F, const float* K,
                         int32_t k_per_frame, const float* Rt, int32_t rt_per_frame, int32_t H, int32_t W, int32_t S, float near,
                         bool tex, RenderAASource src, int32_t C, const float* bg, int32_t bg_per_frame, float* proj, uint64_t* key,
                         float* out, float* alpha, float* depth, void* stream) {
  ARG(verts && vi && K && Rt && src.data && src.tab && (!tex || src.vt) && proj && key && out && alpha, "%s: null argument", who);
  ARG(V >= 1 && F >= 1 && (int64_t)F * 3 <= 0x7fffffff, "%s: V=%d, F=%d: need V >= 1, 1 <= 3 F < 2^31", who, V, F);
  CHK(render_samples(who, H, W, S, near));
  int64_t pblocks;
  CHK(render_pixel_grid(who, N, C, H, W, &pblocks));
  CHK(render_mesh_grid(who, N, V, F));
  CHK(render_distinct(who, {proj, key, out, alpha, depth}, {verts, vi, K, Rt, src.data, src.tab, src.vt, bg}));
  if (N == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  CHK(render_front(nullptr, verts, V, vi, F, N, K, k_per_frame, Rt, rt_per_frame, H, W, S, near, proj, key, s));
  const auto resolve = tex ? render_aa_kernel<true> : render_aa_kernel<false>;
  resolve<<<(unsigned)(N * pblocks), RENDER_THREADS, 0, s>>>(proj, V, vi, (const unsigned long long*)key, H, W, S, (int)pblocks, src, C, bg,
                                                             bg_per_frame ? (int64_t)C * H * W : 0, out, alpha, depth);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_render_antialiased_texture(const float* verts, int64_t N, int32_t V, const int32_t* vi, int32_t F, const float* vt,
                                              int32_t T, const int32_t* vti, const float* K, int32_t k_per_frame, const float* Rt,
                                              int32_t rt_per_frame, int32_t H, int32_t W, int32_t S, float near, const float* tex,
                                              int32_t tex_per_frame, int32_t C, int32_t Ht, int32_t Wt, int32_t flip_v, const float* bg,
                                              int32_t bg_per_frame, float* proj, uint64_t* key, float* out, float* alpha, void* stream) {
  const char* who = "render_antialiased_texture";
  ARG(T >= 1, "%s: T=%d: need T >= 1", who, T);
  ARG(Ht >= 1 && Wt >= 1 && (int64_t)Ht * Wt <= 0x7fffffff, "%s: a %d x %d texture: need 1 <= Ht Wt < 2^31", who, Ht, Wt);
  const RenderAASource src = {tex, tex_per_frame ? (int64_t)C * Ht * Wt : 0, vt, vti, Ht, Wt, flip_v};
  return render_aa_run(who, verts, N, V, vi, F, K, k_per_frame, Rt, rt_per_frame, H, W, S, near, true, src, C, bg, bg_per_frame, proj,
                       key, out, alpha, nullptr, stream);
}

extern "C" int a2p_render_antialiased_values(const float* verts, int64_t N, int32_t V, const int32_t* vi, int32_t F, const float* K,
                                             int32_t k_per_frame, const float* Rt, int32_t rt_per_frame, int32_t H, int32_t W, int32_t S,
                                             float near, const float* values, int32_t C, const float* bg, int32_t bg_per_frame,
                                             float* proj, uint64_t* key, float* out, float* alpha, float* depth, void* stream) {
  const RenderAASource src = {values, (int64_t)V * C, nullptr, vi, 0, 0, 0};
  return render_aa_run("render_antialiased_values", verts, N, V, vi, F, K, k_per_frame, Rt, rt_per_frame, H, W, S, near, false, src, C,
                       bg, bg_per_frame, proj, key, out, alpha, depth, stream);
}
