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
  CHK(render_samples(who, H, W, S, near));
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
  CHK(render_mesh_grid(who, N, sumV, sumF));
  const SceneBody* b = d.body;                                       // entries P.. repeat the last body: they add no array
  CHK(render_distinct(who, {proj, key, out, alpha, depth, body_alpha},
                      {faces, K, Rt, bg, b[0].verts, b[0].place, b[0].tex, b[0].vt, b[0].vti, b[1].verts, b[1].place, b[1].tex, b[1].vt, b[1].vti,
                       b[2].verts, b[2].place, b[2].tex, b[2].vt, b[2].vti, b[3].verts, b[3].place, b[3].tex, b[3].vt, b[3].vti}));
  if (N == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  CHK(render_front(&d, nullptr, d.V, faces, d.F, N, K, k_per_frame, Rt, rt_per_frame, H, W, S, near, proj, key, s));
  scene_resolve_kernel<<<(unsigned)(N * pblocks), RENDER_THREADS, 0, s>>>(d, proj, faces, (const unsigned long long*)key, H, W, S,
                                                                          (int)pblocks, C, bg, bg_per_frame ? (int64_t)C * H * W : 0, out,
                                                                          alpha, depth, body_alpha);
  HIPCHK(hipGetLastError());
  return 0;
}
