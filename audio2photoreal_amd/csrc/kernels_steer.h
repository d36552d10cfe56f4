// Steering joints to 3D targets (audio2photoreal_amd/sample/steer.py, BodySkeleton.solve_ik): the loss of a frame's skeleton
// against reach / aim constraints, its gradient with respect to the pose parameters -- a backward pass through
// skin_states_kernel's solve (kernels_skin.h) -- and a few steps of descent in the sampler's normalised space, as ONE launch for
// all N frames.  fp32; one workgroup per frame; every sum runs in a fixed order and nothing is accumulated with atomics, so a
// frame's result does not depend on N or on its index, and two runs give the same bits (the rule of kernels_skin.h).
//
// LDS of a workgroup (dynamic): st [J][8] + loc [J][8] + x [P_pos + P_scale] + z [P_pos] + g [P_pos] + red [2 SKIN_THREADS] +
// seed [16][8] floats; J = 1024, P = 1024: 32 + 32 + 4 + 4 + 4 + 2 + 0.5 = 78.5 KiB of the CU's 160 KiB (the body model's
// J = 160, P = 116: 11.6 KiB).  More than 64 KiB needs hipFuncAttributeMaxDynamicSharedMemorySize (a2p_steer.h sets it).
//
// The two [J][8] arrays change their meaning as a pass goes on, which is what keeps the budget at two of them:
//   forward    st = global state (t, q xyzw, s), skin_states_kernel's arithmetic in its order
//              loc = local state as (t, Euler angles r, s, -): the local quaternion pre (x) fromXYZ(r) is recomputed from r
//   backward   levels from the deepest to the roots; joint j of the level (one thread) sums, in this order, its constraint
//              seeds (ascending k) and its children's contributions (ascending child index) into the adjoint of its global
//              state, and at the same time turns each child's global adjoint into the adjoints of that child's 7 joint
//              parameters.  Then st[j] = global adjoint (the state of j is not read again: its children are done), loc[c] =
//              parameter adjoints of child c (7 values).  The roots' local state is their global state.
// The transposed parameter transform then reads loc through the compressed COLUMNS, one thread per parameter, ascending row.
#pragma once
#include "kernels_skin.h"

#define STEER_MAX_CONSTRAINTS 16
#define STEER_REACH 0
#define STEER_AIM 1

struct SteerP {
  // frame n = b * T + t reads z from za (and zu) at b * in_seq + t * in_row; zu non-NULL: z = fmaf(cfg[b], a - u, u), the guided
  // output of the two sequence blocks of a step (cfg_combine); the result goes to oa (and ou) at b * out_seq + t * out_row
  const float* za;
  const float* zu;
  const float* cfg;
  float* oa;
  float* ou;
  int64_t in_seq, in_row, out_seq, out_row;
  int T;
  const float* mean;      // [P_pos] or NULL (0)
  const float* std;       // [P_pos] or NULL (1)
  const float* scale;     // [N or 1][P_scale]
  int64_t scale_stride;
  int P_pos, P_scale, J, n_levels;
  const int* row_ptr; const int* cols; const float* vals;          // parameter transform, compressed rows (all P columns)
  const int* col_ptr; const int* rows; const float* cvals;         // the same, compressed columns (the P_pos pose columns)
  const float* offsets; const float* joint_offset; const float* pre_rotation;
  const int* parents; const int* order; const int* level_start;
  const int* child_ptr; const int* child_idx;                      // children of joint j: child_idx[child_ptr[j] .. child_ptr[j + 1]), ascending
  float gx, gy, gz;       // global_scaling
  int K;
  int joint[STEER_MAX_CONSTRAINTS];
  int kind[STEER_MAX_CONSTRAINTS];
  float axis[STEER_MAX_CONSTRAINTS][3];
  const float* targets;   // [N][K][3]
  const float* weights;   // [N][K]
  float alpha, max_step;
  int iterations;
  float* loss;            // [N] or NULL: the loss before the first iteration
  float* grad;            // [N][P_pos] or NULL: its gradient with respect to z
};

__device__ __forceinline__ SkinQuat steer_conj(const SkinQuat q) { return SkinQuat{-q.x, -q.y, -q.z, q.w}; }

// d (skin_qrot(q, v) . g) / d q
__device__ __forceinline__ SkinQuat steer_qrot_adj_q(const SkinQuat q, const SkinVec v, const SkinVec g) {
  const float av = q.x * v.x + q.y * v.y + q.z * v.z, ag = q.x * g.x + q.y * g.y + q.z * g.z, vg = v.x * g.x + v.y * g.y + v.z * g.z;
  const float cx = v.y * g.z - v.z * g.y, cy = v.z * g.x - v.x * g.z, cz = v.x * g.y - v.y * g.x;   // v x g
  SkinQuat o;
  o.x = 2.0f * (q.w * cx + g.x * av + v.x * ag - 2.0f * q.x * vg);
  o.y = 2.0f * (q.w * cy + g.y * av + v.y * ag - 2.0f * q.y * vg);
  o.z = 2.0f * (q.w * cz + g.z * av + v.z * ag - 2.0f * q.z * vg);
  o.w = 2.0f * (q.x * cx + q.y * cy + q.z * cz);                                                  // g . (a x v) = a . (v x g)
  return o;
}

// fromXYZ of skin_states_kernel and its derivatives with respect to the three half angles
__device__ __forceinline__ SkinQuat steer_from_xyz(float r0, float r1, float r2, SkinQuat* d0, SkinQuat* d1, SkinQuat* d2) {
  const float h0 = -0.5f * r0, h1 = 0.5f * r1, h2 = 0.5f * r2;
  const float c0 = cosf(h0), c1 = cosf(h1), c2 = cosf(h2), s0 = sinf(h0), s1 = sinf(h1), s2 = sinf(h2);
  SkinQuat e;
  e.x = -s0 * (c1 * c2) - c0 * (s1 * s2);
  e.y = c0 * (s1 * c2) - s0 * (c1 * s2);
  e.z = c0 * (c1 * s2) + s0 * (s1 * c2);
  e.w = c0 * (c1 * c2) - s0 * (s1 * s2);
  if (d0) {
    *d0 = SkinQuat{-e.w, -e.z, e.y, e.x};
    *d1 = SkinQuat{s0 * (s1 * c2) - c0 * (c1 * s2), c0 * (c1 * c2) + s0 * (s1 * s2), s0 * (c1 * c2) - c0 * (s1 * s2),
                   -c0 * (s1 * c2) - s0 * (c1 * s2)};
    *d2 = SkinQuat{-e.y, e.x, e.w, -e.z};
  }
  return e;
}

// adjoints of a joint's local state (t, q, s) -> adjoints of its 7 joint parameters, written over loc[j] = (t, r, s, -)
__device__ __forceinline__ void steer_local_adjoint(float* lc, const float* pre_rotation, int j, const SkinVec at, const SkinQuat aq,
                                                    float as) {
  const SkinQuat pre = {pre_rotation[4 * j], pre_rotation[4 * j + 1], pre_rotation[4 * j + 2], pre_rotation[4 * j + 3]};
  SkinQuat d0, d1, d2;
  steer_from_xyz(lc[3], lc[4], lc[5], &d0, &d1, &d2);
  const SkinQuat ae = skin_qmul(steer_conj(pre), aq);   // q = pre (x) e
  const float ls = lc[6];
  lc[0] = at.x;
  lc[1] = at.y;
  lc[2] = at.z;
  lc[3] = -0.5f * (ae.x * d0.x + ae.y * d0.y + ae.z * d0.z + ae.w * d0.w);
  lc[4] = 0.5f * (ae.x * d1.x + ae.y * d1.y + ae.z * d1.z + ae.w * d1.w);
  lc[5] = 0.5f * (ae.x * d2.x + ae.y * d2.y + ae.z * d2.z + ae.w * d2.w);
  lc[6] = as * ls * 0.69314718055994531f;               // s = exp2(v)
}

// sum (mode 0) or maximum (mode 1) over the workgroup of one value per thread, in a fixed order; every thread gets the result
__device__ __forceinline__ float steer_reduce(float v, float* red, int tid, int mode) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = SKIN_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = mode ? fmaxf(red[tid], red[tid + s]) : red[tid] + red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// Grid N, SKIN_THREADS threads, dynamic LDS (16 J + P + 2 P_pos + 2 SKIN_THREADS + 8 STEER_MAX_CONSTRAINTS) floats.
//   theta = mean + std z;  L = sum_k reach: w/2 |p - y|^2, aim: w (1 - rot(q_j, a) . d), p = global_scaling t_j,
//   d = (y - p) / |y - p| held constant (0 and no gradient when y = p);  g = std dL/dtheta;
//   `iterations` times  z <- z - min(alpha L / |g|^2, max_step / |g|inf) g;  L = 0, |g| = 0 or anything non-finite: z stays.
// A frame whose weights are all zero leaves z, reports L = 0 and g = 0, and does not write oa / ou when they alias the input
// (the caller's two sequence blocks keep their own values: the step tail then computes what it computes without steering).
__global__ __launch_bounds__(SKIN_THREADS) void skin_steer_kernel(const SteerP p) {
  extern __shared__ float skin_lds[];
  const int J = p.J, P_pos = p.P_pos, P = p.P_pos + p.P_scale, K = p.K;
  float* st = skin_lds;                     // [J][8]
  float* loc = st + (int64_t)J * 8;         // [J][8]
  float* x = loc + (int64_t)J * 8;          // [P]
  float* z = x + P;                         // [P_pos]
  float* g = z + P_pos;                     // [P_pos]
  float* red = g + P_pos;                   // [2 SKIN_THREADS]
  float* seed = red + 2 * SKIN_THREADS;     // [STEER_MAX_CONSTRAINTS][8]: adjoint of (t, q) of the constraint's joint, and its loss term
  const int tid = threadIdx.x;
  const int64_t n = blockIdx.x;
  const int64_t b = n / p.T, t = n - b * p.T;
  const float* za = p.za + b * p.in_seq + t * p.in_row;
  const float* zu = p.zu ? p.zu + b * p.in_seq + t * p.in_row : nullptr;
  float* oa = p.oa + b * p.out_seq + t * p.out_row;
  float* ou = p.ou ? p.ou + b * p.out_seq + t * p.out_row : nullptr;
  const float* tg = p.targets + n * K * 3;
  const float* wt = p.weights + n * K;

  bool any = false;
  for (int k = 0; k < K; ++k) any |= !(wt[k] == 0.0f);
  if (!any) {
    if (oa != za)
      for (int i = tid; i < P_pos; i += SKIN_THREADS) {
        const float v = zu ? fmaf(p.cfg[b], za[i] - zu[i], zu[i]) : za[i];
        oa[i] = v;
        if (ou) ou[i] = v;
      }
    if (p.loss && tid == 0) p.loss[n] = 0.0f;
    if (p.grad)
      for (int i = tid; i < P_pos; i += SKIN_THREADS) p.grad[n * P_pos + i] = 0.0f;
    return;
  }

  for (int i = tid; i < P_pos; i += SKIN_THREADS) z[i] = zu ? fmaf(p.cfg[b], za[i] - zu[i], zu[i]) : za[i];
  for (int i = tid; i < p.P_scale; i += SKIN_THREADS) x[P_pos + i] = p.scale[n * p.scale_stride + i];
  __syncthreads();

  const int passes = p.iterations > 0 ? p.iterations : 1;
  for (int it = 0; it < passes; ++it) {
    // ---------------------------------------------------------------- forward: skin_states_kernel
    for (int i = tid; i < P_pos; i += SKIN_THREADS) x[i] = (p.mean ? p.mean[i] : 0.0f) + (p.std ? p.std[i] : 1.0f) * z[i];
    __syncthreads();
    for (int j = tid; j < J; j += SKIN_THREADS) {
      float v[7];
#pragma unroll
      for (int c = 0; c < 7; ++c) {
        const int r = 7 * j + c;
        float a = 0.0f;
        for (int e = p.row_ptr[r]; e < p.row_ptr[r + 1]; ++e) a += p.vals[e] * x[p.cols[e]];
        v[c] = a + p.offsets[r];
      }
      const SkinQuat e = steer_from_xyz(v[3], v[4], v[5], nullptr, nullptr, nullptr);
      const SkinQuat pre = {p.pre_rotation[4 * j], p.pre_rotation[4 * j + 1], p.pre_rotation[4 * j + 2], p.pre_rotation[4 * j + 3]};
      const SkinQuat q = skin_qmul(pre, e);
      float* o = st + 8 * j;
      float* lc = loc + 8 * j;
      o[0] = lc[0] = v[0] + p.joint_offset[3 * j];
      o[1] = lc[1] = v[1] + p.joint_offset[3 * j + 1];
      o[2] = lc[2] = v[2] + p.joint_offset[3 * j + 2];
      o[3] = q.x;
      o[4] = q.y;
      o[5] = q.z;
      o[6] = q.w;
      o[7] = lc[6] = exp2f(v[6]);
      lc[3] = v[3];
      lc[4] = v[4];
      lc[5] = v[5];
    }
    __syncthreads();
    for (int l = 1; l < p.n_levels; ++l) {
      const int lo = p.level_start[l], hi = p.level_start[l + 1];
      for (int i = lo + tid; i < hi; i += SKIN_THREADS) {
        const int j = p.order[i];
        const float* pa = st + 8 * p.parents[j];
        float* o = st + 8 * j;
        const SkinQuat pq = {pa[3], pa[4], pa[5], pa[6]};
        const float ps = pa[7];
        const SkinQuat lq = {o[3], o[4], o[5], o[6]};
        const SkinVec lt = {o[0] * ps, o[1] * ps, o[2] * ps};
        const SkinQuat gq = skin_qmul(pq, lq);
        const SkinVec gt = skin_qrot(pq, lt);
        o[0] = gt.x + pa[0];
        o[1] = gt.y + pa[1];
        o[2] = gt.z + pa[2];
        o[3] = gq.x;
        o[4] = gq.y;
        o[5] = gq.z;
        o[6] = gq.w;
        o[7] = ps * o[7];
      }
      __syncthreads();
    }

    // ---------------------------------------------------------------- loss terms and their seeds: one thread per constraint
    for (int k = tid; k < K; k += SKIN_THREADS) {
      const float* s = st + 8 * p.joint[k];
      const float w = wt[k];
      const float px = p.gx * s[0], py = p.gy * s[1], pz = p.gz * s[2];
      const float ex = px - tg[3 * k], ey = py - tg[3 * k + 1], ez = pz - tg[3 * k + 2];
      float* sd = seed + 8 * k;
      sd[0] = sd[1] = sd[2] = sd[3] = sd[4] = sd[5] = sd[6] = sd[7] = 0.0f;
      if (p.kind[k] == STEER_REACH) {
        sd[0] = w * ex * p.gx;
        sd[1] = w * ey * p.gy;
        sd[2] = w * ez * p.gz;
        sd[7] = 0.5f * w * (ex * ex + ey * ey + ez * ez);
      } else {
        const float len = sqrtf(ex * ex + ey * ey + ez * ez);
        if (len > 0.0f) {
          const SkinVec d = {-ex / len, -ey / len, -ez / len};
          const SkinQuat q = {s[3], s[4], s[5], s[6]};
          const SkinVec a = {p.axis[k][0], p.axis[k][1], p.axis[k][2]};
          const SkinVec r = skin_qrot(q, a);
          const SkinQuat aq = steer_qrot_adj_q(q, a, SkinVec{-w * d.x, -w * d.y, -w * d.z});
          sd[3] = aq.x;
          sd[4] = aq.y;
          sd[5] = aq.z;
          sd[6] = aq.w;
          sd[7] = w * (1.0f - (r.x * d.x + r.y * d.y + r.z * d.z));
        }
      }
    }
    __syncthreads();
    float L = 0.0f;
    for (int k = 0; k < K; ++k) L += seed[8 * k + 7];

    // ---------------------------------------------------------------- backward: deepest level first
    for (int l = p.n_levels - 1; l >= 0; --l) {
      const int lo = p.level_start[l], hi = p.level_start[l + 1];
      for (int i = lo + tid; i < hi; i += SKIN_THREADS) {
        const int j = p.order[i];
        float* o = st + 8 * j;
        const SkinQuat q = {o[3], o[4], o[5], o[6]};
        const float s = o[7];
        SkinVec at = {0.0f, 0.0f, 0.0f};
        SkinQuat aq = {0.0f, 0.0f, 0.0f, 0.0f};
        float as = 0.0f;
        for (int k = 0; k < K; ++k)
          if (p.joint[k] == j) {
            const float* sd = seed + 8 * k;
            at.x += sd[0]; at.y += sd[1]; at.z += sd[2];
            aq.x += sd[3]; aq.y += sd[4]; aq.z += sd[5]; aq.w += sd[6];
          }
        for (int e = p.child_ptr[j]; e < p.child_ptr[j + 1]; ++e) {
          const int c = p.child_idx[e];
          const float* ca = st + 8 * c;       // the child's global adjoint
          float* lc = loc + 8 * c;            // its local state (t, r, s)
          const SkinVec ct = {ca[0], ca[1], ca[2]};
          const SkinQuat cq = {ca[3], ca[4], ca[5], ca[6]};
          const float cs = ca[7];
          const SkinQuat pre = {p.pre_rotation[4 * c], p.pre_rotation[4 * c + 1], p.pre_rotation[4 * c + 2], p.pre_rotation[4 * c + 3]};
          const SkinQuat lq = skin_qmul(pre, steer_from_xyz(lc[3], lc[4], lc[5], nullptr, nullptr, nullptr));
          const SkinVec lt = {lc[0], lc[1], lc[2]};
          const float ls = lc[6];
          // child: q_c = q (x) lq, t_c = rot(q, lt s) + t, s_c = s ls
          const SkinVec v = {lt.x * s, lt.y * s, lt.z * s};
          const SkinVec av = skin_qrot(steer_conj(q), ct);                 // adjoint of v: the transposed rotation
          const SkinQuat rq = steer_qrot_adj_q(q, v, ct);
          const SkinQuat mq = skin_qmul(cq, steer_conj(lq));               // adjoint of q through the product
          at.x += ct.x; at.y += ct.y; at.z += ct.z;
          aq.x += rq.x + mq.x; aq.y += rq.y + mq.y; aq.z += rq.z + mq.z; aq.w += rq.w + mq.w;
          as += (av.x * lt.x + av.y * lt.y + av.z * lt.z) + cs * ls;
          steer_local_adjoint(lc, p.pre_rotation, c, SkinVec{av.x * s, av.y * s, av.z * s}, skin_qmul(steer_conj(q), cq), cs * s);
        }
        if (l == 0) {
          steer_local_adjoint(loc + 8 * j, p.pre_rotation, j, at, aq, as);
        } else {
          o[0] = at.x; o[1] = at.y; o[2] = at.z;
          o[3] = aq.x; o[4] = aq.y; o[5] = aq.z; o[6] = aq.w;
          o[7] = as;
        }
      }
      __syncthreads();
    }

    // ---------------------------------------------------------------- transposed parameter transform, g = std dL/dtheta
    float g2 = 0.0f, gm = 0.0f;
    for (int i = tid; i < P_pos; i += SKIN_THREADS) {
      float a = 0.0f;
      for (int e = p.col_ptr[i]; e < p.col_ptr[i + 1]; ++e) {
        const int r = p.rows[e];
        a += p.cvals[e] * loc[8 * (r / 7) + r % 7];
      }
      a *= p.std ? p.std[i] : 1.0f;
      g[i] = a;
      g2 += a * a;
      gm = fmaxf(gm, fabsf(a));
      if (it == 0 && p.grad) p.grad[n * P_pos + i] = a;
    }
    if (it == 0 && p.loss && tid == 0) p.loss[n] = L;
    if (p.iterations == 0) break;
    g2 = steer_reduce(g2, red, tid, 0);
    gm = steer_reduce(gm, red + SKIN_THREADS, tid, 1);
    // (fmaxf drops a nan: g2 carries it)
    if (L > 0.0f && g2 > 0.0f && L <= 3.4028234e38f && g2 <= 3.4028234e38f) {
      const float step = fminf(p.alpha * L / g2, p.max_step / gm);
      for (int i = tid; i < P_pos; i += SKIN_THREADS) z[i] -= step * g[i];
    }
    __syncthreads();
  }

  for (int i = tid; i < P_pos; i += SKIN_THREADS) {
    oa[i] = z[i];
    if (ou) ou[i] = z[i];
  }
}
