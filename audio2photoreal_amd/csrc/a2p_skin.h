// C ABI of the posed body geometry (include/a2p_hip.h "posed geometry"; kernels in kernels_skin.h).  Context-free like the
// motion evaluation: the skeleton tables are device arrays the caller built once (audio2photoreal_amd/skinning.py validates
// them on the host).  Included at the end of a2p_lib.hip (set_err / ARG / HIPCHK).
#pragma once

extern "C" int a2p_skin_states(const float* pose, const float* scale, int32_t scale_per_frame, int64_t N, int32_t P_pos,
                               int32_t P_scale, int32_t J, const int32_t* row_ptr, const int32_t* cols, const float* vals,
                               const float* offsets, const float* joint_offset, const float* pre_rotation, const int32_t* parents,
                               const int32_t* order, const int32_t* level_start, int32_t n_levels, const float* inv_bind,
                               float* states, float* mats, void* stream) {
  static_assert(SKIN_MAX_JOINTS == A2P_SKIN_MAX_JOINTS && SKIN_MAX_PARAMS == A2P_SKIN_MAX_PARAMS &&
                    SKIN_MAX_INFLUENCES == A2P_SKIN_MAX_INFLUENCES, "skinning limits");
  ARG(pose && row_ptr && cols && vals && offsets && joint_offset && pre_rotation && parents && order && level_start && inv_bind,
      "skin_states: null argument");
  ARG(states || mats, "skin_states: both outputs are null");
  ARG(J >= 1 && J <= A2P_SKIN_MAX_JOINTS, "skin_states: J=%d outside [1, %d]", J, A2P_SKIN_MAX_JOINTS);
  ARG(P_pos >= 1 && P_scale >= 0 && P_pos + (int64_t)P_scale <= A2P_SKIN_MAX_PARAMS,
      "skin_states: need P_pos >= 1, P_scale >= 0, P_pos + P_scale <= %d (got %d + %d)", A2P_SKIN_MAX_PARAMS, P_pos, P_scale);
  ARG(P_scale == 0 || scale, "skin_states: P_scale=%d but scale is null", P_scale);
  ARG(n_levels >= 1 && n_levels <= J, "skin_states: n_levels=%d outside [1, J=%d]", n_levels, J);
  ARG(N >= 0 && N <= 0x7fffffff, "skin_states: N=%lld outside [0, 2^31)", (long long)N);
  if (N == 0) return 0;
  const size_t lds = ((size_t)8 * J + P_pos + P_scale + 12 * SKIN_THREADS) * sizeof(float);   // <= 48 KiB
  skin_states_kernel<<<(unsigned)N, SKIN_THREADS, lds, (hipStream_t)stream>>>(
      pose, scale, scale_per_frame ? (int64_t)P_scale : 0, P_pos, P_scale, J, row_ptr, cols, vals, offsets, joint_offset,
      pre_rotation, parents, order, level_start, n_levels, inv_bind, states, mats);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_skin_vertices(const float* mats, int64_t N, int32_t J, const float* base, const float* unposed,
                                 int32_t unposed_per_frame, const int32_t* idx, const float* w, int32_t V, int32_t K, float gx,
                                 float gy, float gz, float* out, void* stream) {
  ARG(mats && base && idx && w && out, "skin_vertices: null argument");
  ARG(J >= 1 && J <= A2P_SKIN_MAX_JOINTS, "skin_vertices: J=%d outside [1, %d]", J, A2P_SKIN_MAX_JOINTS);
  ARG(K >= 1 && K <= A2P_SKIN_MAX_INFLUENCES, "skin_vertices: K=%d outside [1, %d]", K, A2P_SKIN_MAX_INFLUENCES);
  ARG(V >= 1 && (int64_t)V * K <= 0x7fffffff, "skin_vertices: V=%d, K=%d: need V >= 1 and V K < 2^31", V, K);
  const int tiles = (V + SKIN_VTILE - 1) / SKIN_VTILE;
  ARG(N >= 0 && N * tiles <= 0x7fffffff, "skin_vertices: N=%lld frames x %d vertex tiles exceed the grid", (long long)N, tiles);
  ARG(out != mats && out != base && out != unposed, "skin_vertices: out must not alias an input");
  if (N == 0) return 0;
  const size_t lds = ((size_t)12 * J + 3 * SKIN_THREADS) * sizeof(float);   // <= 51 KiB
  skin_vertices_kernel<<<(unsigned)(N * tiles), SKIN_THREADS, lds, (hipStream_t)stream>>>(
      mats, J, base, unposed, unposed_per_frame ? (int64_t)V * 3 : 0, idx, w, V, K, tiles, gx, gy, gz, out);
  HIPCHK(hipGetLastError());
  return 0;
}
