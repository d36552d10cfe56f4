// DPM-Solver++(2M) (Lu et al. 2022, multistep, data prediction): the step tails of the multistep sampler.  Phase 1 is the
// phase 1 of step_tail_kernel / windowed_step_tail_kernel (the CFG combine u + scale * (a - u), the non-finite flag, the 32 x 33
// LDS transpose); phase 2 replaces the DDIM / DDPM update with
//   x_next = CX x + B x0 + P x0_prev
// from the host's fp32 coefficient table coefs [A2P_NMS, n_steps] (GaussianDiffusion.multistep_table, rows a2p_ms_coef_id).
// One extra fp32 read per element (x0_prev) against the DDIM tail, no noise read.
#pragma once
#include "a2p_common.h"
#include "kernels_misc.h"
#include "kernels_window.h"

enum { MS_CX = 0, MS_B1, MS_B2, MS_P2 };

// The update in a fixed order of explicit fused multiply-adds, so a host restatement can match it bit for bit:
//   with history     fmaf(CX, x, fmaf(B2, x0, P2 * x0_prev))
//   without history  fmaf(CX, x, B1 * x0)              (first step of a call, skip_timesteps, order 1)
// Row 0 (sigma' = 0) returns x0 itself: the last step's sample is its pred_xstart, signed zeros and all.
__device__ __forceinline__ float multistep_update(float x, float x0, float x0p, bool hist, const float* cf, int ns, int t) {
#pragma clang fp contract(off)
  if (t == 0) return x0;
  const float cx = cf[MS_CX * ns + t];
  if (!hist) return fmaf(cx, x, cf[MS_B1 * ns + t] * x0);
  return fmaf(cx, x, fmaf(cf[MS_B2 * ns + t], x0, cf[MS_P2 * ns + t] * x0p));
}

struct MsStepP {
  const float* mo;        // model output rows of the B (cond) + B (uncond) sequences: mo[(seq*mo_seq_rows + t) * C + c]
  int64_t mo_seq_rows;
  int B, C, Tn;
  const float* scale;     // [B]
  const float* x;         // [B,C,T]
  const int64_t* t_idx;   // [B]
  const float* coefs;     // [A2P_NMS, n_steps]
  int n_steps;
  const float* x0_prev;   // [B,C,T] the previous step's pred_xstart, or NULL (first-order step)
  int clip;
  const float* known;     // [B,C,T] held values, or NULL (plain step)
  const uint8_t* mask;    // [B,C,T] 1 = held, or NULL
  float* x_next;          // [B,C,T] (may alias x)
  float* x0;              // [B,C,T] pred_xstart (never aliases x0_prev)
  int* nonfinite;
};

// Grid (ceil(T / 32), ceil(C / 32), B), 256 threads, as step_tail_kernel / inpaint_step_tail_kernel.  Held elements replace x0
// after the clamp (kernels_inpaint.h); a non-finite held value ORs the flag too.
__global__ __launch_bounds__(256) void multistep_step_tail_kernel(MsStepP p) {
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
  const bool hist = p.x0_prev != nullptr;
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    if (c >= p.C || t >= p.Tn) continue;
    float x0 = tile[tx][i];
    if (p.clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    const int64_t o = ((int64_t)b * p.C + c) * p.Tn + t;
    if (p.mask && p.mask[o]) {
      x0 = p.known[o];
      bad |= !(fabsf(x0) <= 3.4028234e38f);
    }
    const float xv = p.x[o];
    const float pv = hist ? p.x0_prev[o] : 0.f;
    p.x0[o] = x0;
    p.x_next[o] = multistep_update(xv, x0, pv, hist, p.coefs, p.n_steps, ts);
  }
  if (bad && p.nonfinite) atomicOr(p.nonfinite, 1);
}

struct MsWinStepP {
  const float* mo;        // model output rows of the R*W (cond) + R*W (uncond) sequences
  int64_t mo_seq_rows;
  int R, W, C, Tw, Ttot;
  const float* scale;     // [R*W]
  const float* weights;   // [W, Tw] blend weights
  const float* x;         // [R*W, C, Tw]
  const int64_t* t_idx;   // [R*W]
  const float* coefs;     // [A2P_NMS, n_steps]
  int n_steps;
  const float* x0_prev;   // [R*W, C, Tw] or NULL: read from the first covering window, like x
  int clip;
  float* x_next;          // [R*W, C, Tw]
  float* x0;              // [R*W, C, Tw] pred_xstart
  float* x_glob;          // [R, C, Ttot] or NULL
  float* x0_glob;         // [R, C, Ttot] or NULL
  int* nonfinite;
  int starts[WIN_MAX];
};

// Grid (ceil(Ttot / 32), ceil(C / 32), R), 256 threads: windowed_step_tail_kernel's blend over the covering windows in ascending w,
// then the multistep update once per global frame; the same bits go to every window copy and to the global outputs.
__global__ __launch_bounds__(256) void windowed_multistep_step_tail_kernel(MsWinStepP p) {
  __shared__ float tile[32][33];  // [t][c]
  const int r = blockIdx.z, t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int B = p.R * p.W;
  bool bad = false;
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    float acc = 0.f;
    if (t < p.Ttot && c < p.C) {
      bool first = true;
      for (int w = 0; w < p.W; ++w) {
        const int lt = t - p.starts[w];
        if (lt < 0) break;
        if (lt >= p.Tw) continue;
        const int b = r * p.W + w;
        const float a = p.mo[((int64_t)b * p.mo_seq_rows + lt) * p.C + c];
        const float u = p.mo[((int64_t)(B + b) * p.mo_seq_rows + lt) * p.C + c];
        const float g = u + p.scale[b] * (a - u);
        bad |= !(fabsf(g) <= 3.4028234e38f);
        const float v = p.weights[(int64_t)w * p.Tw + lt] * g;
        acc = first ? v : acc + v;
        first = false;
      }
    }
    tile[i][tx] = acc;
  }
  if (bad && p.nonfinite) atomicOr(p.nonfinite, 1);
  __syncthreads();
  const bool hist = p.x0_prev != nullptr;
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    if (c >= p.C || t >= p.Ttot) continue;
    float x0 = tile[tx][i];
    if (p.clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    int w0 = 0;
    while (t - p.starts[w0] >= p.Tw) ++w0;
    const int b0 = r * p.W + w0;
    const int64_t o0 = ((int64_t)b0 * p.C + c) * p.Tw + (t - p.starts[w0]);
    const int ts = (int)p.t_idx[b0];
    const float xv = p.x[o0];
    const float pv = hist ? p.x0_prev[o0] : 0.f;
    const float xn = multistep_update(xv, x0, pv, hist, p.coefs, p.n_steps, ts);
    for (int w = w0; w < p.W; ++w) {
      const int lt = t - p.starts[w];
      if (lt < 0) break;
      const int64_t o = ((int64_t)(r * p.W + w) * p.C + c) * p.Tw + lt;
      p.x_next[o] = xn;
      p.x0[o] = x0;
    }
    const int64_t og = ((int64_t)r * p.C + c) * p.Ttot + t;
    if (p.x_glob) p.x_glob[og] = xn;
    if (p.x0_glob) p.x0_glob[og] = x0;
  }
}

// stand-alone elementwise form (x, x0, x0_prev, out all [B, per_sample]; out may alias x)
__global__ void multistep_update_kernel(const float* x, const float* x0, const float* x0p, const int64_t* t_idx, const float* cf, int ns,
                                        int64_t per, int64_t total, float* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int t = (int)t_idx[i / per];
  out[i] = multistep_update(x[i], x0[i], x0p ? x0p[i] : 0.f, x0p != nullptr, cf, ns, t);
}
