// C ABI of the surface maps (include/a2p_hip.h "surface maps"; kernels in kernels_surface.h).  Context-free like the posed
// geometry: the topology tables are device arrays the caller built once (audio2photoreal_amd/surface.py validates them on the
// host).  Included at the end of a2p_lib.hip (set_err / ARG / HIPCHK).
#pragma once

static inline int surface_tiles(int64_t n) { return (int)((n + SURFACE_THREADS - 1) / SURFACE_THREADS); }

extern "C" int a2p_surface_normals(const float* verts, int64_t N, int32_t V, const int32_t* vi, int32_t F, const int32_t* inc_ptr,
                                   const int32_t* inc_face, const float* camera, int32_t camera_per_frame, float* normals,
                                   float* view_cos, void* stream) {
  static_assert(SURFACE_MAX_UV == A2P_SURFACE_MAX_UV && SURFACE_MAX_CHANNELS == A2P_SURFACE_MAX_CHANNELS, "surface limits");
  static_assert(3ll * SURFACE_MAX_UV * SURFACE_MAX_UV <= 0x7fffffffll, "3 H H must fit in int32");
  ARG(verts && vi && inc_ptr && inc_face, "surface_normals: null argument");
  ARG(normals || view_cos, "surface_normals: both outputs are null");
  ARG(!view_cos || camera, "surface_normals: view_cos needs a camera");
  ARG(V >= 1 && F >= 1 && (int64_t)F * 3 <= 0x7fffffff, "surface_normals: V=%d, F=%d: need V >= 1, 1 <= 3 F < 2^31", V, F);
  const int tiles = surface_tiles(V);
  ARG(N >= 0 && N * tiles <= 0x7fffffff, "surface_normals: N=%lld frames x %d vertex tiles exceed the grid", (long long)N, tiles);
  ARG(normals != verts && view_cos != verts && (!normals || (const float*)normals != camera) &&
          (!view_cos || ((const float*)view_cos != camera && view_cos != normals)),
      "surface_normals: an output must not alias an input or the other output");
  if (N == 0) return 0;
  surface_normals_kernel<<<(unsigned)(N * tiles), SURFACE_THREADS, 0, (hipStream_t)stream>>>(
      verts, V, tiles, vi, inc_ptr, inc_face, camera, camera_per_frame ? 3 : 0, normals, view_cos);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_surface_to_uv(const float* values, int64_t N, int32_t V, int32_t C, const int32_t* index_image,
                                 const float* bary_image, int32_t H, float* out, void* stream) {
  ARG(values && index_image && bary_image && out, "surface_to_uv: null argument");
  ARG(V >= 1, "surface_to_uv: V=%d, need V >= 1", V);
  ARG(C >= 1 && C <= A2P_SURFACE_MAX_CHANNELS, "surface_to_uv: C=%d outside [1, %d]", C, A2P_SURFACE_MAX_CHANNELS);
  ARG(H >= 1 && H <= A2P_SURFACE_MAX_UV, "surface_to_uv: uv_size=%d outside [1, %d]", H, A2P_SURFACE_MAX_UV);
  const int64_t HH = (int64_t)H * H, tblocks = surface_tiles(HH);
  ARG(N >= 0 && N <= 0x7fffffff, "surface_to_uv: N=%lld outside [0, 2^31)", (long long)N);
  const int64_t groups = (N + SURFACE_FRAME_GROUP - 1) / SURFACE_FRAME_GROUP;
  ARG(groups * tblocks <= 0x7fffffff, "surface_to_uv: %lld frame groups x %lld texel blocks exceed the grid", (long long)groups,
      (long long)tblocks);
  ARG(out != values && (const float*)out != bary_image && (const void*)out != (const void*)index_image,
      "surface_to_uv: out must not alias an input");
  if (N == 0) return 0;
  surface_to_uv_kernel<<<(unsigned)(groups * tblocks), SURFACE_THREADS, 0, (hipStream_t)stream>>>(
      values, N, V, C, index_image, bary_image, HH, tblocks, out);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_surface_from_uv(const float* values_uv, int64_t N, int32_t C, int32_t Hs, int32_t Ws, const float* vt, int32_t T,
                                   const int32_t* v2uv, int32_t V, float* out, void* stream) {
  ARG(values_uv && vt && v2uv && out, "surface_from_uv: null argument");
  ARG(C >= 1 && V >= 1 && T >= 1, "surface_from_uv: C=%d, V=%d, T=%d: each must be >= 1", C, V, T);
  ARG(Hs >= 1 && Ws >= 1 && (int64_t)Hs * Ws <= 0x7fffffff, "surface_from_uv: a %d x %d plane: need 1 <= H' W' < 2^31", Hs, Ws);
  const int tiles = surface_tiles(V);
  ARG(N >= 0 && N * tiles <= 0x7fffffff, "surface_from_uv: N=%lld frames x %d vertex tiles exceed the grid", (long long)N, tiles);
  ARG(out != values_uv && (const float*)out != vt && (const void*)out != (const void*)v2uv, "surface_from_uv: out must not alias an input");
  if (N == 0) return 0;
  surface_from_uv_kernel<<<(unsigned)(N * tiles), SURFACE_THREADS, 0, (hipStream_t)stream>>>(values_uv, C, Hs, Ws, vt, v2uv, V,
                                                                                            tiles, out);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_surface_uv_index(const float* vt, int32_t T, const int32_t* vti, const int32_t* vi, int32_t F, int32_t H,
                                    int32_t* index_image, float* bary_image, int32_t* face_image, void* stream) {
  ARG(vt && vti && vi && index_image && bary_image && face_image, "surface_uv_index: null argument");
  ARG(T >= 1 && F >= 1 && (int64_t)F * 3 <= 0x7fffffff, "surface_uv_index: T=%d, F=%d: need T >= 1, 1 <= 3 F < 2^31", T, F);
  ARG(H >= 1 && H <= A2P_SURFACE_MAX_UV, "surface_uv_index: uv_size=%d outside [1, %d]", H, A2P_SURFACE_MAX_UV);
  ARG((void*)index_image != (void*)bary_image && index_image != face_image && (void*)bary_image != (void*)face_image,
      "surface_uv_index: the three images must be distinct");
  ARG((const void*)index_image != (const void*)vt && index_image != vti && index_image != vi && (const float*)bary_image != vt &&
          (const void*)bary_image != (const void*)vti && (const void*)bary_image != (const void*)vi &&
          (const void*)face_image != (const void*)vt && face_image != vti && face_image != vi,
      "surface_uv_index: an image must not alias an input");
  const int64_t HH = (int64_t)H * H;
  hipStream_t s = (hipStream_t)stream;
  surface_fill_kernel<<<(unsigned)surface_tiles(HH), SURFACE_THREADS, 0, s>>>(face_image, HH, INT_MAX);
  surface_uv_cover_kernel<<<(unsigned)((F + 3) / 4), SURFACE_THREADS, 0, s>>>(vt, vti, F, H, face_image);
  surface_uv_resolve_kernel<<<(unsigned)surface_tiles(HH), SURFACE_THREADS, 0, s>>>(vt, vti, vi, H, index_image, bary_image,
                                                                                  face_image);
  HIPCHK(hipGetLastError());
  return 0;
}
