// Posed body geometry (audio2photoreal_amd/skinning.py): the first stage of the reference's renderer, visualize/ca_body/utils/
// lbs.py -- parameter transform, hierarchical skeleton solve (solve_skeleton_state), states_to_matrix against the bind state, and
// linear blend skinning -- as two launches for all N frames.  fp32 like the reference; every sum runs in a fixed order and
// nothing is accumulated with atomics, and a frame is computed by its own workgroup(s) from its own inputs only: its result
// does not depend on N or on its index, and two runs give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SKIN_MAX_JOINTS 1024    // states of one frame in LDS: 1024 x 8 fp32 = 32 KiB
#define SKIN_MAX_PARAMS 1024    // pose + scale parameters of one frame in LDS
#define SKIN_MAX_INFLUENCES 16
#define SKIN_THREADS 256
#define SKIN_VTILE 1024         // vertices of one workgroup of skin_vertices_kernel (4 per thread)

struct SkinQuat {
  float x, y, z, w;
};
struct SkinVec {
  float x, y, z;
};

// Quaternion.batchMul (xyzw)
__device__ __forceinline__ SkinQuat skin_qmul(const SkinQuat q, const SkinQuat r) {
  SkinQuat o;
  o.x = q.x * r.w + q.y * r.z - q.z * r.y + q.w * r.x;
  o.y = -q.x * r.z + q.y * r.w + q.z * r.x + q.w * r.y;
  o.z = q.x * r.y - q.y * r.x + q.z * r.w + q.w * r.z;
  o.w = -q.x * r.x - q.y * r.y - q.z * r.z + q.w * r.w;
  return o;
}

// Quaternion.batchRot: v + 2 (w (a x v) + a x (a x v)), a = q.xyz
__device__ __forceinline__ SkinVec skin_qrot(const SkinQuat q, const SkinVec v) {
  const float ax = q.y * v.z - q.z * v.y, ay = q.z * v.x - q.x * v.z, az = q.x * v.y - q.y * v.x;
  const float bx = q.y * az - q.z * ay, by = q.z * ax - q.x * az, bz = q.x * ay - q.y * ax;
  SkinVec o;
  o.x = v.x + 2.0f * (ax * q.w + bx);
  o.y = v.y + 2.0f * (ay * q.w + by);
  o.z = v.z + 2.0f * (az * q.w + bz);
  return o;
}

// Grid N, SKIN_THREADS threads, dynamic LDS (8 J + P + 12 SKIN_THREADS) floats: one frame per workgroup.
//   x = cat(pose[n], scale[n or 0])                                     [P = P_pos + P_scale] in LDS
//   value[r] = sum over the non-zeros of row r of the parameter transform (ascending column) + offsets[r]      r = 7 j + c
//   local: t = value[0:3] + joint_offset[j], q = pre_rotation[j] (x) fromXYZ(value[3:6]), s = exp2(value[6])
//   levels: level 0 holds the roots (global = local); the joints of level l (order[level_start[l] .. level_start[l + 1]))
//   have their parents in earlier levels: q = parent_q (x) q, t = rot(parent_q, t parent_s) + parent_t, s = parent_s s.
//   states [N, J, 8] (t, q xyzw, s) and mats [N, J, 3, 4] = [R(q (x) bind_q^-1) s / bind_s | rot(q, bind_t' s) + t], with
//   inv_bind [J, 8] = (bind_t' = rot(bind_q^-1, -bind_t) / bind_s, bind_q^-1, 1 / bind_s) computed once on the host.
// Either output may be NULL.
__global__ __launch_bounds__(SKIN_THREADS) void skin_states_kernel(
    const float* __restrict__ pose, const float* __restrict__ scale, int64_t scale_stride, int P_pos, int P_scale, int J,
    const int* __restrict__ row_ptr, const int* __restrict__ cols, const float* __restrict__ vals,
    const float* __restrict__ offsets, const float* __restrict__ joint_offset, const float* __restrict__ pre_rotation,
    const int* __restrict__ parents, const int* __restrict__ order, const int* __restrict__ level_start, int n_levels,
    const float* __restrict__ inv_bind, float* __restrict__ states, float* __restrict__ mats) {
  extern __shared__ float skin_lds[];
  float* st = skin_lds;               // [J][8]
  float* x = st + (int64_t)J * 8;     // [P]
  float* stage = x + P_pos + P_scale; // [SKIN_THREADS][12]
  const int tid = threadIdx.x;
  const int64_t n = blockIdx.x;
  for (int i = tid; i < P_pos; i += SKIN_THREADS) x[i] = pose[n * P_pos + i];
  for (int i = tid; i < P_scale; i += SKIN_THREADS) x[P_pos + i] = scale[n * scale_stride + i];
  __syncthreads();

  for (int j = tid; j < J; j += SKIN_THREADS) {
    float v[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      const int r = 7 * j + c;
      float a = 0.0f;
      for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e) a += vals[e] * x[cols[e]];
      v[c] = a + offsets[r];
    }
    const float h0 = -0.5f * v[3], h1 = 0.5f * v[4], h2 = 0.5f * v[5];
    const float c0 = cosf(h0), c1 = cosf(h1), c2 = cosf(h2), s0 = sinf(h0), s1 = sinf(h1), s2 = sinf(h2);
    SkinQuat e;
    e.x = -s0 * (c1 * c2) - c0 * (s1 * s2);
    e.y = c0 * (s1 * c2) - s0 * (c1 * s2);
    e.z = c0 * (c1 * s2) + s0 * (s1 * c2);
    e.w = c0 * (c1 * c2) - s0 * (s1 * s2);
    const SkinQuat pre = {pre_rotation[4 * j], pre_rotation[4 * j + 1], pre_rotation[4 * j + 2], pre_rotation[4 * j + 3]};
    const SkinQuat q = skin_qmul(pre, e);
    float* o = st + 8 * j;
    o[0] = v[0] + joint_offset[3 * j];
    o[1] = v[1] + joint_offset[3 * j + 1];
    o[2] = v[2] + joint_offset[3 * j + 2];
    o[3] = q.x;
    o[4] = q.y;
    o[5] = q.z;
    o[6] = q.w;
    o[7] = exp2f(v[6]);
  }
  __syncthreads();

  for (int l = 1; l < n_levels; ++l) {
    const int lo = level_start[l], hi = level_start[l + 1];
    for (int i = lo + tid; i < hi; i += SKIN_THREADS) {
      const int j = order[i];
      const float* p = st + 8 * parents[j];
      float* o = st + 8 * j;
      const SkinQuat pq = {p[3], p[4], p[5], p[6]};
      const float ps = p[7];
      const SkinQuat lq = {o[3], o[4], o[5], o[6]};
      const SkinVec lt = {o[0] * ps, o[1] * ps, o[2] * ps};
      const SkinQuat gq = skin_qmul(pq, lq);
      const SkinVec gt = skin_qrot(pq, lt);
      o[0] = gt.x + p[0];
      o[1] = gt.y + p[1];
      o[2] = gt.z + p[2];
      o[3] = gq.x;
      o[4] = gq.y;
      o[5] = gq.z;
      o[6] = gq.w;
      o[7] = ps * o[7];
    }
    __syncthreads();
  }

  if (states) {
    float* out = states + n * J * 8;
    for (int i = tid; i < J * 8; i += SKIN_THREADS) out[i] = st[i];
  }
  if (!mats) return;
  for (int base = 0; base < J; base += SKIN_THREADS) {
    const int j = base + tid;
    if (j < J) {
      const float* s = st + 8 * j;
      const float* b = inv_bind + 8 * j;
      const SkinQuat q = {s[3], s[4], s[5], s[6]};
      const SkinQuat br = {b[3], b[4], b[5], b[6]};
      const SkinQuat tr = skin_qmul(q, br);
      const float ts = s[7] * b[7];
      const SkinVec bt = {b[0] * s[7], b[1] * s[7], b[2] * s[7]};
      const SkinVec r = skin_qrot(q, bt);
      const float twx = 2.0f * tr.x * tr.w, twy = 2.0f * tr.y * tr.w, twz = 2.0f * tr.z * tr.w;
      const float txx = 2.0f * tr.x * tr.x, txy = 2.0f * tr.y * tr.x, txz = 2.0f * tr.z * tr.x;
      const float tyy = 2.0f * tr.y * tr.y, tyz = 2.0f * tr.z * tr.y, tzz = 2.0f * tr.z * tr.z;
      float* m = stage + 12 * tid;
      m[0] = (1.0f - (tyy + tzz)) * ts;
      m[1] = (txy - twz) * ts;
      m[2] = (txz + twy) * ts;
      m[3] = r.x + s[0];
      m[4] = (txy + twz) * ts;
      m[5] = (1.0f - (txx + tzz)) * ts;
      m[6] = (tyz - twx) * ts;
      m[7] = r.y + s[1];
      m[8] = (txz - twy) * ts;
      m[9] = (tyz + twx) * ts;
      m[10] = (1.0f - (txx + tyy)) * ts;
      m[11] = r.z + s[2];
    }
    __syncthreads();
    const int cnt = min(SKIN_THREADS, J - base) * 12;
    float* out = mats + (n * J + base) * 12;
    for (int i = tid; i < cnt; i += SKIN_THREADS) out[i] = stage[i];
    __syncthreads();
  }
}

// Grid N * tiles (tiles = ceil(V / SKIN_VTILE); block b is tile b % tiles of frame n = b / tiles), SKIN_THREADS threads, dynamic
// LDS (12 J + 3 SKIN_THREADS) floats.  The workgroup loads the J matrices of frame n into LDS; a thread owns one vertex of each
// 256-vertex sub-tile:
//   p = base[v] (+ unposed[n or 0][v]);  out[n][v] = (sum over k = 0 .. K - 1 of w[k][v] (M[idx[k][v]] [p, 1])) * gscale
// idx / w are stored [K, V] (a wave reads 64 consecutive entries); unused slots hold index 0 and weight 0.  The three
// coordinates go through an LDS tile so the workgroup stores 768 consecutive floats.
__global__ __launch_bounds__(SKIN_THREADS) void skin_vertices_kernel(
    const float* __restrict__ mats, int J, const float* __restrict__ base, const float* __restrict__ unposed,
    int64_t unposed_stride, const int* __restrict__ idx, const float* __restrict__ w, int V, int K, int tiles, float gx, float gy,
    float gz, float* __restrict__ out) {
  extern __shared__ float skin_lds[];
  float* m = skin_lds;                     // [J][12]
  float* tile = m + (int64_t)J * 12;       // [SKIN_THREADS][3]
  const int tid = threadIdx.x;
  const int64_t n = blockIdx.x / tiles;
  const int vt = blockIdx.x % tiles;
  const float* mg = mats + n * J * 12;
  for (int i = tid; i < J * 12; i += SKIN_THREADS) m[i] = mg[i];
  __syncthreads();
  const int v_end = min(V, (vt + 1) * SKIN_VTILE);
  for (int v0 = vt * SKIN_VTILE; v0 < v_end; v0 += SKIN_THREADS) {
    const int v = v0 + tid;
    if (v < V) {
      float px = base[3 * (int64_t)v], py = base[3 * (int64_t)v + 1], pz = base[3 * (int64_t)v + 2];
      if (unposed) {
        const float* u = unposed + n * unposed_stride + 3 * (int64_t)v;
        px = u[0] + px;
        py = u[1] + py;
        pz = u[2] + pz;
      }
      float ax = 0.0f, ay = 0.0f, az = 0.0f;
      for (int k = 0; k < K; ++k) {
        const int j = idx[(int64_t)k * V + v];
        const float wk = w[(int64_t)k * V + v];
        const float* a = m + 12 * j;
        ax += wk * (a[0] * px + a[1] * py + a[2] * pz + a[3]);
        ay += wk * (a[4] * px + a[5] * py + a[6] * pz + a[7]);
        az += wk * (a[8] * px + a[9] * py + a[10] * pz + a[11]);
      }
      tile[3 * tid] = ax * gx;
      tile[3 * tid + 1] = ay * gy;
      tile[3 * tid + 2] = az * gz;
    }
    __syncthreads();
    const int cnt = min(SKIN_THREADS, V - v0) * 3;
    float* o = out + (n * V + v0) * 3;
    for (int i = tid; i < cnt; i += SKIN_THREADS) o[i] = tile[i];
    __syncthreads();
  }
}
