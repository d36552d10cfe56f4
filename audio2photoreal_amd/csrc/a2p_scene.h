// C ABI of the multi-body scene render (include/a2p_hip.h "scenes of several bodies"; kernels in kernels_scene.h).  Context-free like
// the rendered images: the per-body tables and the merged face table are device arrays the caller built once
// (audio2photoreal_amd/scene.py).  Included at the end of a2p_lib.hip after a2p_render.h (render_tiles, render_pixel_grid).
#pragma once

extern "C" int a2p_scene_render(const a2p_scene_body* bodies, int32_t P, const int32_t* faces, int64_t N, const float* K,
                                int32_t k_per_frame, const float* Rt, int32_t rt_per_frame, int32_t H, int32_t W, int32_t S, float near,
                                int32_t C, const float* bg, int32_t bg_per_frame, float* proj, uint64_t* key, float* out, float* alpha,
                                float* depth, float* body_alpha, void* stream) {
  static_assert(SCENE_MAX_BODIES == A2P_SCENE_MAX_BODIES, "scene limits");
  const char* who = "scene_render";
  ARG(bodies && faces && K && Rt && proj && key && out && alpha && depth && body_alpha, "%s: null argument", who);
  ARG(P >= 1 && P <= A2P_SCENE_MAX_BODIES, "%s: P=%d bodies: need 1 <= P <= %d", who, P, A2P_SCENE_MAX_BODIES);
  ARG(S >= 1 && S <= A2P_RENDER_MAX_SUPERSAMPLE, "%s: S=%d samples per axis: need 1 <= S <= %d", who, S, A2P_RENDER_MAX_SUPERSAMPLE);
  ARG(H >= 1 && W >= 1 && (int64_t)S * H <= A2P_RENDER_MAX_SIZE && (int64_t)S * W <= A2P_RENDER_MAX_SIZE,
      "%s: a %d x %d image at S=%d: need 1 <= H, W and S H, S W <= %d", who, H, W, S, A2P_RENDER_MAX_SIZE);
  ARG(near > 0.0f && near < __builtin_inff(), "%s: near=%g: need a positive finite distance", who, (double)near);
  int64_t pblocks;
  CHK(render_pixel_grid(who, N, C, H, W, &pblocks));
  SceneDesc d = {};
  int64_t sumV = 0, sumF = 0;
  for (int p = 0; p < P; ++p) {
    const a2p_scene_body& b = bodies[p];
    ARG(b.verts && b.tex && b.vt && b.vti, "%s: body %d: null argument", who, p);
    ARG(b.V >= 1 && b.F >= 1 && b.T >= 1, "%s: body %d: V=%d, F=%d, T=%d: need V, F, T >= 1", who, p, b.V, b.F, b.T);
    ARG(b.Ht >= 1 && b.Wt >= 1 && (int64_t)b.Ht * b.Wt <= 0x7fffffff, "%s: body %d: a %d x %d texture: need 1 <= Ht Wt < 2^31", who, p, b.Ht,
        b.Wt);
    SceneBody& o = d.body[p];
    o.verts = b.verts, o.place = b.placement, o.tex = b.tex, o.vt = b.vt, o.vti = b.vti;
    o.place_stride = b.placement_per_frame ? 12 : 0;
    o.tex_stride = b.tex_per_frame ? (int64_t)C * b.Ht * b.Wt : 0;
    o.V = b.V, o.v0 = (int)sumV, o.f0 = (int)sumF;
    o.Ht = b.Ht, o.Wt = b.Wt, o.flip_v = b.flip_v;
    sumV += b.V, sumF += b.F;
    ARG(sumF * 3 <= 0x7fffffff && sumV * 3 <= 0x7fffffff, "%s: the bodies up to %d hold %lld vertices and %lld faces: need 3 sum V, 3 sum F < 2^31",
        who, p, (long long)sumV, (long long)sumF);
  }
  for (int p = P; p < SCENE_MAX_BODIES; ++p) {                       // never selected: the compare chains stop below these starts
    d.body[p] = d.body[P - 1];
    d.body[p].v0 = d.body[p].f0 = 0x7fffffff;
  }
  d.P = P, d.V = (int)sumV, d.F = (int)sumF;
  const int64_t vtiles = render_tiles(sumV), fblocks = render_tiles(sumF), sH = (int64_t)S * H, sW = (int64_t)S * W;
  ARG(N * vtiles <= 0x7fffffff && N * fblocks <= 0x7fffffff, "%s: N=%lld frames x %lld vertex tiles or %lld face blocks exceed the grid", who,
      (long long)N, (long long)vtiles, (long long)fblocks);
  const void* outs[] = {proj, key, out, alpha, depth, body_alpha};
  for (int a = 0; a < 6; ++a) {
    const void* shared[] = {faces, K, Rt, bg};
    for (int b = 0; b < 4; ++b) ARG(outs[a] != shared[b], "%s: a scratch or output array must not alias an input", who);
    for (int p = 0; p < P; ++p) {
      const void* ins[] = {bodies[p].verts, bodies[p].placement, bodies[p].tex, bodies[p].vt, bodies[p].vti};
      for (int b = 0; b < 5; ++b) ARG(outs[a] != ins[b], "%s: a scratch or output array must not alias an input", who);
    }
    for (int b = 0; b < a; ++b) ARG(outs[a] != outs[b], "%s: the scratch and output arrays must be distinct", who);
  }
  if (N == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  scene_project_kernel<<<(unsigned)(N * vtiles), RENDER_THREADS, 0, s>>>(d, (int)vtiles, K, k_per_frame ? 9 : 0, Rt, rt_per_frame ? 12 : 0,
                                                                         (float)S, proj);
  HIPCHK(hipMemsetAsync(key, 0xff, (size_t)(N * sH * sW) * sizeof(uint64_t), s));
  render_cover_kernel<<<(unsigned)(N * fblocks), RENDER_THREADS, 0, s>>>(proj, d.V, faces, d.F, (int)fblocks, (int)sH, (int)sW, near,
                                                                         (unsigned long long*)key);
  scene_resolve_kernel<<<(unsigned)(N * pblocks), RENDER_THREADS, 0, s>>>(d, proj, faces, (const unsigned long long*)key, H, W, S,
                                                                          (int)pblocks, C, bg, bg_per_frame ? (int64_t)C * H * W : 0, out,
                                                                          alpha, depth, body_alpha);
  HIPCHK(hipGetLastError());
  return 0;
}
