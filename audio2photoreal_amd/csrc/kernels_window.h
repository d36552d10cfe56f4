// Windowed joint sampling of recordings longer than the denoisers' window (sample/long_form.py): W overlapping windows of T_w
// frames cover T_total global frames, the R repetitions x W windows run as one batch of R*W sequences (b = r * W + w) through
// the ordinary forward, and after every step one kernel reconciles the windows -- for every global frame, the guided x0
// predictions of the covering windows are blended with fixed weights, the posterior update is computed ONCE from the blend, and
// the same bits go to every window copy of that frame.  With the noise drawn per global frame, every copy of a shared frame
// then holds identical bits after every step.
#pragma once
#include "a2p_common.h"
#include "kernels_misc.h"

#define WIN_MAX 256   // A2P_WINDOW_MAX (a2p_hip.h): the window starts travel in the kernel arguments

struct WinStepP {
  const float* mo;        // model output rows of the R*W (cond) + R*W (uncond) sequences: mo[(seq*mo_seq_rows + t) * C + c]
  int64_t mo_seq_rows;
  int R, W, C, Tw, Ttot;
  const float* scale;     // [R*W]
  const float* weights;   // [W, Tw] blend weights; the covering windows' weights of a frame sum to 1
  int sampler;            // 0 ddim, 1 ddpm
  const float* x;         // [R*W, C, Tw]
  const int64_t* t_idx;   // [R*W]
  const float* tables;
  int n_steps;
  const float* noise;     // [R, C, Ttot] or NULL
  float eta;
  int clip;
  float* x_next;          // [R*W, C, Tw]
  float* x0;              // [R*W, C, Tw] pred_xstart
  float* x_glob;          // [R, C, Ttot] or NULL
  float* x0_glob;         // [R, C, Ttot] or NULL
  int* nonfinite;
  int starts[WIN_MAX];    // ascending, starts[0] = 0, starts[W-1] + Tw = Ttot, no gaps
};

// Grid (ceil(Ttot / 32), ceil(C / 32), R), 256 threads.  Phase 1 reads the model output rows channel-contiguous (as
// step_tail_kernel does) and blends over the covering windows in ascending w; phase 2 writes frame-contiguous rows.
__global__ __launch_bounds__(256) void windowed_step_tail_kernel(WinStepP p) {
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
        if (lt < 0) break;                     // ascending starts: no later window covers t either
        if (lt >= p.Tw) continue;
        const int b = r * p.W + w;
        const float a = p.mo[((int64_t)b * p.mo_seq_rows + lt) * p.C + c];
        const float u = p.mo[((int64_t)(B + b) * p.mo_seq_rows + lt) * p.C + c];
        const float g = u + p.scale[b] * (a - u);
        bad |= !(fabsf(g) <= 3.4028234e38f);
        const float v = p.weights[(int64_t)w * p.Tw + lt] * g;
        acc = first ? v : acc + v;             // no 0 + v: with one window (weight 1) the bits are g's, -0 included
        first = false;
      }
    }
    tile[i][tx] = acc;
  }
  if (bad && p.nonfinite) atomicOr(p.nonfinite, 1);
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    if (c >= p.C || t >= p.Ttot) continue;
    float x0 = tile[tx][i];
    if (p.clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    int w0 = 0;
    while (t - p.starts[w0] >= p.Tw) ++w0;     // first covering window (the starts cover [0, Ttot))
    const int b0 = r * p.W + w0;
    const int64_t o0 = ((int64_t)b0 * p.C + c) * p.Tw + (t - p.starts[w0]);
    const int ts = (int)p.t_idx[b0];
    const float xv = p.x[o0];
    const int64_t og = ((int64_t)r * p.C + c) * p.Ttot + t;
    const float nv = p.noise ? p.noise[og] : 0.f;
    const float xn = p.sampler == 0 ? ddim_update(x0, xv, nv, p.tables, p.n_steps, ts, p.eta)
                                    : ddpm_update(x0, xv, nv, p.tables, p.n_steps, ts);
    for (int w = w0; w < p.W; ++w) {
      const int lt = t - p.starts[w];
      if (lt < 0) break;
      const int64_t o = ((int64_t)(r * p.W + w) * p.C + c) * p.Tw + lt;
      p.x_next[o] = xn;
      p.x0[o] = x0;
    }
    if (p.x_glob) p.x_glob[og] = xn;
    if (p.x0_glob) p.x0_glob[og] = x0;
  }
}

struct WinGatherP {
  const float* src;       // [R, rows_per_seq, Ttot * k] (rows_per_seq = ch for channels first) or [R, Ttot * k * ch]
  float* dst;             // [R*W, rows_per_seq, Tw * k] or [R*W, Tw * k * ch]
  int R, W, rows;         // rows = channels for channels first, else 1
  int64_t src_len, dst_len, unit;  // per row: source elements, window elements, elements per frame
  int starts[WIN_MAX];
};

// One (window sequence, row) pair per blockIdx.y, a contiguous run of dst_len elements copied from source offset
// start * unit; grid-stride along the run, so consecutive lanes touch consecutive addresses on both sides.
__global__ __launch_bounds__(256) void window_gather_kernel(WinGatherP p) {
  const int seq = blockIdx.y / p.rows, row = blockIdx.y - seq * p.rows;
  const int r = seq / p.W, w = seq - r * p.W;
  const float* s = p.src + ((int64_t)r * p.rows + row) * p.src_len + (int64_t)p.starts[w] * p.unit;
  float* d = p.dst + ((int64_t)seq * p.rows + row) * p.dst_len;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.dst_len; i += (int64_t)gridDim.x * blockDim.x) d[i] = s[i];
}
