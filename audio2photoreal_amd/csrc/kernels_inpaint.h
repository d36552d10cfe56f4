// Sampling with held elements (sample/inpaint.py): MDM's x0 replacement.  After the guided model output is formed, the held
// elements of the x0 prediction are overwritten with the caller's values, and the DDIM / DDPM update then runs as usual.  This
// is step_tail_kernel's CFG + sampler path with one extra read per element; the held values enter neither the clamp nor the
// model's non-finite test of the guided output, but a non-finite held value ORs the same flag.
#pragma once
#include "a2p_common.h"
#include "kernels_misc.h"

struct InpaintStepP {
  const float* mo;        // model output rows of the B (cond) + B (uncond) sequences: mo[(seq*mo_seq_rows + t) * C + c]
  int64_t mo_seq_rows;
  int B, C, Tn;
  const float* scale;     // [B]
  int sampler;            // 0 ddim, 1 ddpm
  const float* x;         // [B,C,T]
  const int64_t* t_idx;   // [B]
  const float* tables;
  int n_steps;
  const float* noise;     // [B,C,T] or NULL
  float eta;
  int clip;
  const float* known;     // [B,C,T] held values (normalised, x's layout)
  const uint8_t* mask;    // [B,C,T] 1 = held
  float* x_next;          // [B,C,T] (may alias x)
  float* x0;              // [B,C,T] pred_xstart or NULL
  int* nonfinite;
};

// Grid (ceil(T / 32), ceil(C / 32), B), 256 threads: phase 1 reads the model output channel-contiguous into the 32 x 33 tile
// (as step_tail_kernel), phase 2 reads x, noise, known and mask and writes frame-contiguous rows.
__global__ __launch_bounds__(256) void inpaint_step_tail_kernel(InpaintStepP p) {
  __shared__ float tile[32][33];  // [t][c]
  const int b = blockIdx.z, t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const float sc = p.scale[b];
  bool bad = false;
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    float g = 0.f;
    if (t < p.Tn && c < p.C) {
      const float a = p.mo[((int64_t)b * p.mo_seq_rows + t) * p.C + c];
      const float u = p.mo[((int64_t)(p.B + b) * p.mo_seq_rows + t) * p.C + c];
      g = u + sc * (a - u);
      bad |= !(fabsf(g) <= 3.4028234e38f);
    }
    tile[i][tx] = g;
  }
  __syncthreads();
  const int ts = (int)p.t_idx[b];
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    if (c >= p.C || t >= p.Tn) continue;
    float x0 = tile[tx][i];
    if (p.clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    const int64_t o = ((int64_t)b * p.C + c) * p.Tn + t;
    if (p.mask[o]) {
      x0 = p.known[o];
      bad |= !(fabsf(x0) <= 3.4028234e38f);
    }
    const float xv = p.x[o];
    const float nv = p.noise ? p.noise[o] : 0.f;
    if (p.x0) p.x0[o] = x0;
    p.x_next[o] = p.sampler == 0 ? ddim_update(x0, xv, nv, p.tables, p.n_steps, ts, p.eta)
                                 : ddpm_update(x0, xv, nv, p.tables, p.n_steps, ts);
  }
  if (bad && p.nonfinite) atomicOr(p.nonfinite, 1);
}
