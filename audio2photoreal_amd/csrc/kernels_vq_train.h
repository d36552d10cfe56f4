// One training step of the residual-VQ tokenizer (train/train_vq.py ModelTrainer.run_train_step on model/vqvae.py
// TemporalVertexCodec.forward in training mode): forward, SmoothL1 losses, backward, AdamW, EMA codebook update.  State, activations and
// elementwise arithmetic are fp32; dot products and row sums accumulate in double and round once.
//
// Five launches per step, whatever the shapes (host side: a2p_vq_train.h):
//   vqt_norms_kernel   |embed|^2 per code of the books as they stand at the start of the step
//   vqt_fwd_bwd_kernel one workgroup per sequence: encoder, residual quantisation, decoder, losses, backward-data.  Every conv's
//                      input activation and output gradient goes to the workspace, tokens and per-level residuals with them
//   vqt_wgrad_kernel   weight and bias gradients: one fixed-order sum over the B (T + 7) rows per parameter element
//   vqt_stats_kernel   one wave per (level, code): rows that picked the code, in ascending order -> EMA of cluster_size / embed_avg
//   vqt_update_kernel  embed = embed_avg / smoothed cluster_size, the loss record, AdamW
// No float atomics: every sum has one order, so a step is bit-reproducible.
//
// Gradient of the quantiser (straight-through, `residual - quantized` NOT detached): only level 0 carries commitment gradient,
//   dL/dz = dL/d(decoder input) + commit / depth * 2 (z - q_0) / (B T e);   levels >= 1 give loss value, tokens and statistics.
#pragma once
#include "a2p_common.h"

// workspace slots of [R][e] floats per sequence (R = T + 7): inputs of the ten convs and gradients of their pre-activations
enum {
  VQT_A0 = 0, VQT_A1, VQT_A2, VQT_A3,              // encoder.enc.{0,2,4,6} after LeakyReLU
  VQT_DIN, VQT_D0, VQT_D1, VQT_D2, VQT_D3,          // decoder input (7 zero rows + quantised latents), decoder.dec.{0,2,4,6} after LeakyReLU
  VQT_GE0, VQT_GE1, VQT_GE2, VQT_GE3, VQT_GE4,      // dL/d(output of encoder.enc.{0,2,4,6,8}) before the activation
  VQT_GD0, VQT_GD1, VQT_GD2, VQT_GD3,               // the same for decoder.dec.{0,2,4,6}; dec.8's is `dpred`
  VQT_SLOTS
};
#define VQT_SLOT_X (-1)      // the batch itself (7 zero rows in front)
#define VQT_SLOT_DPRED (-2)  // [T][nv]

struct VqTrainP {
  const float* x;            // [B][T][nv]
  float* params;             // flat: encoder.enc.*, decoder.project_mean_shape.*, decoder.dec.* in parameters() order
  float* m1;                 // AdamW exp_avg, same layout
  float* m2;                 // AdamW exp_avg_sq
  float* grads;              // same layout (the project_mean_shape range is never written)
  float* embed[8];
  float* embed_avg[8];
  float* cluster[8];
  int64_t ew[5], eb[5], dw[5], db[5];  // offsets into the flat buffers
  int64_t pms_off, pms_n, n_params;
  int B, T, depth, categories, e, nv;
  float commit, loss_vel;
  float decay, one_minus_decay, eps_ema;
  float lr_wd, step_size, bc2_sqrt;    // lr * weight_decay, lr / bias_correction1, sqrt(bias_correction2)
  float* act;                // [B][VQT_SLOTS][R][e]
  float* pred;               // [B][T][nv]
  float* dpred;              // [B][T][nv]
  float* res;                // [B T][depth][e]: the residual each level quantised
  float* rowcommit;          // [B T][depth]: |residual - code|^2 per row and level
  float* seqloss;            // [B][2]: SmoothL1 sums of the sequence (motion, velocity)
  float* norms;              // [depth][categories]
  float* rawcount;           // [depth][categories]: rows per code in this batch
  int64_t* tokens;           // [B][T][depth]
  float* record;             // [6] accumulated: loss, loss_motion, loss_commit, loss_vel, perplexity, steps
};

__device__ __forceinline__ float vqt_block_sum(float v, float* red) {  // every thread of the 256 calls it; one fixed order
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void vqt_norms_kernel(const VqTrainP p) {
  const int gw = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (gw >= p.depth * p.categories) return;
  const int k = gw / p.categories, c = gw - k * p.categories;
  const float* row = p.embed[k] + (int64_t)c * p.e;
  float s = 0.f;
  for (int i = lane; i < p.e; i += 64) s += row[i] * row[i];
  s = wave_sum(s);
  if (lane == 0) p.norms[gw] = s;
}

// Dot products accumulate in double and are rounded to fp32 once: every stored activation and gradient is then within an ulp of
// its exact value, where an fp32 chain of 64..2000 additions would stack several (the parity gates are a few ulp wide).
__device__ __forceinline__ double vqt_mul(float a, float b) { return (double)a * (double)b; }

// out[r] = act(b + W[:, :, 0] in[r - d] + W[:, :, 1] in[r]) for rows [nf, R); `in` and `out` in LDS, a copy to `save` (nullable)
__device__ __forceinline__ void vqt_conv2_fwd(const float* __restrict__ W, const float* __restrict__ bias, const float* in, float* out,
                                              float* __restrict__ save, int R, int e, int nf, int d, bool act) {
  for (int i = threadIdx.x; i < (R - nf) * e; i += 256) {
    const int r = nf + i / e, co = i % e;
    const float2* w = reinterpret_cast<const float2*>(W + (int64_t)co * e * 2);
    const float* a = in + (r - d) * e;
    const float* b = in + r * e;
    double acc0 = bias[co], acc1 = 0.0;
    for (int ci = 0; ci < e; ci += 2) {
      const float2 w0 = w[ci], w1 = w[ci + 1];
      acc0 += vqt_mul(w0.x, a[ci]) + vqt_mul(w0.y, b[ci]);
      acc1 += vqt_mul(w1.x, a[ci + 1]) + vqt_mul(w1.y, b[ci + 1]);
    }
    float v = (float)(acc0 + acc1);
    if (act) v = act_lrelu02(v);
    out[r * e + co] = v;
    if (save) save[r * e + co] = v;
  }
}

// The transpose: g holds dL/d(out) on rows [fo, R); din rows [fo - d, R).  `mask_act` (the conv's input after its LeakyReLU, as
// saved by the forward) turns din into the gradient of that activation's input.  `add_to`: the decoder's first conv, whose input
// rows 7.. are the latents: din += the commitment term stored there, and the sum (dL/dz) is stored back.
__device__ __forceinline__ void vqt_conv2_bwd(const float* __restrict__ W, const float* g, float* din, int R, int e, int fo, int d,
                                              const float* mask_act, float* save, float* add_to) {
  const int fi = fo - d;
  for (int i = threadIdx.x; i < (R - fi) * e; i += 256) {
    const int r = fi + i / e, ci = i % e;
    const bool hi = r + d < R, lo = r >= fo;
    const float* gh = g + (hi ? r + d : fo) * e;
    const float* gl = g + (lo ? r : fo) * e;
    const float mh = hi ? 1.f : 0.f, ml = lo ? 1.f : 0.f;
    double acc0 = 0.0, acc1 = 0.0;
    for (int co = 0; co < e; co += 2) {
      const float2 w0 = *reinterpret_cast<const float2*>(W + ((int64_t)co * e + ci) * 2);
      const float2 w1 = *reinterpret_cast<const float2*>(W + ((int64_t)(co + 1) * e + ci) * 2);
      acc0 += vqt_mul(mh * w0.x, gh[co]) + vqt_mul(ml * w0.y, gl[co]);
      acc1 += vqt_mul(mh * w1.x, gh[co + 1]) + vqt_mul(ml * w1.y, gl[co + 1]);
    }
    float v = (float)(acc0 + acc1);
    if (mask_act) v *= mask_act[r * e + ci] > 0.f ? 1.f : 0.2f;
    if (add_to && r >= 7) {
      v += add_to[r * e + ci];
      add_to[r * e + ci] = v;
    }
    din[r * e + ci] = v;
    if (save) save[r * e + ci] = v;
  }
}

__device__ __forceinline__ float vqt_sl1(float d) { const float a = fabsf(d); return a < 1.f ? 0.5f * d * d : a - 0.5f; }
__device__ __forceinline__ float vqt_sl1_grad(float d) { return fabsf(d) < 1.f ? d : (d > 0.f ? 1.f : -1.f); }

__global__ __launch_bounds__(256) void vqt_fwd_bwd_kernel(const VqTrainP p) {
  extern __shared__ float sm[];
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int T = p.T, e = p.e, nv = p.nv, R = T + 7, depth = p.depth;
  float* cur = sm;            // [R][e]
  float* nxt = cur + R * e;   // [R][e]
  const float* x = p.x + (int64_t)b * T * nv;
  float* slots = p.act + (int64_t)b * VQT_SLOTS * R * e;
  auto slot = [&](int s) { return slots + (int64_t)s * R * e; };
  const float* P = p.params;
  const int dil[4] = {1, 2, 3, 1};

  // ---- encoder (as vq_encode_kernel): enc.0 is 1x1, a padding row gives LeakyReLU(bias)
  {
    float* save = slot(VQT_A0);
    for (int i = tid; i < R * e; i += 256) {
      const int r = i / e, co = i - r * e;
      double acc0 = P[p.eb[0] + co], acc1 = 0.0;
      if (r >= 7) {
        const float* w = P + p.ew[0] + (int64_t)co * nv;
        const float* xr = x + (int64_t)(r - 7) * nv;
        int ci = 0;
        for (; ci + 1 < nv; ci += 2) { acc0 += vqt_mul(w[ci], xr[ci]); acc1 += vqt_mul(w[ci + 1], xr[ci + 1]); }
        if (ci < nv) acc0 += vqt_mul(w[ci], xr[ci]);
      }
      const float v = act_lrelu02((float)(acc0 + acc1));
      cur[i] = v;
      save[i] = v;
    }
  }
  __syncthreads();
  int first = 0;
  for (int l = 0; l < 4; ++l) {
    const int nf = first + dil[l];
    // enc.8's output (the latents z) is no conv's input: it stays in LDS
    vqt_conv2_fwd(P + p.ew[l + 1], P + p.eb[l + 1], cur, nxt, l < 3 ? slot(VQT_A1 + l) : nullptr, R, e, nf, dil[l], l < 3);
    __syncthreads();
    float* t = cur; cur = nxt; nxt = t;
    first = nf;
  }
  // ---- residual quantisation of rows 7.. of `cur` in place; nxt becomes the decoder input
  for (int i = tid; i < R * e; i += 256) nxt[i] = 0.f;
  __syncthreads();
  const float cscale = p.commit / (float)depth * 2.0f / ((float)p.B * (float)T * (float)e);
  for (int t = wid; t < T; t += 4) {
    float* res = cur + (7 + t) * e;
    float* din = nxt + (7 + t) * e;
    const int64_t row = (int64_t)b * T + t;
    for (int k = 0; k < depth; ++k) {
      float xx = 0.f;
      for (int i = lane; i < e; i += 64) {
        const float v = res[i];
        p.res[(row * depth + k) * e + i] = v;
        xx += v * v;
      }
      xx = wave_sum(xx);
      const float* book = p.embed[k];
      const float* norms = p.norms + (int64_t)k * p.categories;
      float best = INFINITY;
      int bi = p.categories;
      for (int c = lane; c < p.categories; c += 64) {
        const float4* w = reinterpret_cast<const float4*>(book + (int64_t)c * e);
        float dot = 0.f;
        for (int j = 0; j < e / 4; ++j) {
          const float4 a = w[j];
          dot += a.x * res[4 * j] + a.y * res[4 * j + 1] + a.z * res[4 * j + 2] + a.w * res[4 * j + 3];
        }
        const float dist = (xx - 2.0f * dot) + norms[c];  // vq_encode_kernel's expression and tie rule: lowest index wins
        if (dist < best) { best = dist; bi = c; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
      }
      if (bi >= p.categories) bi = 0;
      if (lane == 0) p.tokens[row * depth + k] = bi;
      __builtin_amdgcn_wave_barrier();
      float cs = 0.f;
      for (int i = lane; i < e; i += 64) {
        const float q = book[(int64_t)bi * e + i];
        const float rn = res[i] - q;
        res[i] = rn;
        din[i] += q;
        cs += rn * rn;
        if (k == 0) slot(VQT_GE4)[(7 + t) * e + i] = cscale * rn;  // the commitment term of dL/dz
      }
      cs = wave_sum(cs);
      if (lane == 0) p.rowcommit[row * depth + k] = cs;
      __builtin_amdgcn_wave_barrier();
    }
  }
  __syncthreads();
  {
    float* save = slot(VQT_DIN);
    for (int i = tid; i < R * e; i += 256) save[i] = nxt[i];
  }
  { float* t = cur; cur = nxt; nxt = t; }
  // ---- decoder
  first = 0;
  for (int l = 0; l < 4; ++l) {
    const int nf = first + dil[l];
    vqt_conv2_fwd(P + p.dw[l], P + p.db[l], cur, nxt, slot(VQT_D0 + l), R, e, nf, dil[l], true);
    __syncthreads();
    float* t = cur; cur = nxt; nxt = t;
    first = nf;
  }
  float* pred = p.pred + (int64_t)b * T * nv;
  float* dpred = p.dpred + (int64_t)b * T * nv;
  for (int i = tid; i < T * nv; i += 256) {
    const int t = i / nv, v = i - t * nv;
    const float* w = P + p.dw[4] + (int64_t)v * e;
    const float* a = cur + (7 + t) * e;
    double acc0 = P[p.db[4] + v], acc1 = 0.0;
    for (int ci = 0; ci < e; ci += 2) { acc0 += vqt_mul(w[ci], a[ci]); acc1 += vqt_mul(w[ci + 1], a[ci + 1]); }
    pred[i] = (float)(acc0 + acc1);
  }
  __syncthreads();
  // ---- SmoothL1 (mean reduction, beta 1) of the poses and of their channel differences (the reference's "velocity")
  {
    const float n_all = (float)p.B * (float)T;
    const float gm = 1.0f / (n_all * (float)nv);
    const float gv = nv > 1 ? p.loss_vel / (n_all * (float)(nv - 1)) : 0.f;
    const bool vel = p.loss_vel > 0.f && nv > 1;
    float sm_m = 0.f, sm_v = 0.f;
    for (int i = tid; i < T * nv; i += 256) {
      const int v = i % nv;
      const float d = pred[i] - x[i];
      sm_m += vqt_sl1(d);
      float g = gm * vqt_sl1_grad(d);
      if (vel) {
        if (v + 1 < nv) {
          const float dv = (pred[i] - pred[i + 1]) - (x[i] - x[i + 1]);
          sm_v += vqt_sl1(dv);
          g += gv * vqt_sl1_grad(dv);
        }
        if (v > 0) {
          const float dv = (pred[i - 1] - pred[i]) - (x[i - 1] - x[i]);
          g -= gv * vqt_sl1_grad(dv);
        }
      }
      dpred[i] = g;
    }
    sm_m = vqt_block_sum(sm_m, red);
    sm_v = vqt_block_sum(sm_v, red);
    if (tid == 0) { p.seqloss[2 * b] = sm_m; p.seqloss[2 * b + 1] = sm_v; }
  }
  __syncthreads();
  // ---- backward: dec.8 (1x1), then the four dilated convs of the decoder; cur holds dec.6's activation
  {
    float* save = slot(VQT_GD3);
    const float* w8 = P + p.dw[4];
    for (int i = tid; i < T * e; i += 256) {
      const int t = i / e, ci = i - t * e;
      const float* g = dpred + (int64_t)t * nv;
      double acc0 = 0.0, acc1 = 0.0;
      int v = 0;
      for (; v + 1 < nv; v += 2) { acc0 += vqt_mul(w8[(int64_t)v * e + ci], g[v]); acc1 += vqt_mul(w8[(int64_t)(v + 1) * e + ci], g[v + 1]); }
      if (v < nv) acc0 += vqt_mul(w8[(int64_t)v * e + ci], g[v]);
      const int o = (7 + t) * e + ci;
      const float r = (float)(acc0 + acc1) * (cur[o] > 0.f ? 1.f : 0.2f);
      nxt[o] = r;
      save[o] = r;
    }
  }
  __syncthreads();
  { float* t = cur; cur = nxt; nxt = t; }   // cur: gradient rows [7, R)
  const int fo_of[4] = {1, 3, 6, 7};        // first output row of conv l (dilations 1, 2, 3, 1)
  for (int l = 3; l >= 0; --l) {
    if (l > 0) vqt_conv2_bwd(P + p.dw[l], cur, nxt, R, e, fo_of[l], dil[l], slot(VQT_D0 + l - 1), slot(VQT_GD0 + l - 1), nullptr);
    else vqt_conv2_bwd(P + p.dw[0], cur, nxt, R, e, fo_of[0], dil[0], nullptr, nullptr, slot(VQT_GE4));
    __syncthreads();
    float* t = cur; cur = nxt; nxt = t;
  }
  // ---- encoder backward from dL/dz on rows [7, R) of cur
  for (int l = 3; l >= 0; --l) {
    vqt_conv2_bwd(P + p.ew[l + 1], cur, nxt, R, e, fo_of[l], dil[l], slot(VQT_A0 + l), slot(VQT_GE0 + l), nullptr);
    __syncthreads();
    float* t = cur; cur = nxt; nxt = t;
  }
}

// ---- weight and bias gradients ------------------------------------------------------------------------------------------
struct VqtLayer {
  int64_t w_off, b_off, elem_base;  // elements [elem_base, elem_base + cout cin ks + cout): weights, then biases
  int in_slot, g_slot, cin, cout, ks, dil, fo;
};
struct VqWgradP {
  VqtLayer L[10];
  int64_t total;
  const float* x;
  const float* act;
  const float* dpred;
  float* grads;
  int B, T, e, nv;
};

// 64 parameter elements x 4 segments of the batch per workgroup; the four partial sums are added in segment order
__global__ __launch_bounds__(256) void vqt_wgrad_kernel(const VqWgradP p) {
  __shared__ double part[4][64];
  const int el = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int64_t idx = (int64_t)blockIdx.x * 64 + el;
  const int R = p.T + 7, e = p.e;
  double acc = 0.0;
  int li = 0;
  int64_t j = 0, nW = 0;
  if (idx < p.total) {
    while (li < 9 && idx >= p.L[li + 1].elem_base) ++li;
    const VqtLayer& L = p.L[li];
    j = idx - L.elem_base;
    nW = (int64_t)L.cout * L.cin * L.ks;
    const bool is_w = j < nW;
    int co, ci = 0, shift = 0;
    if (is_w) {
      co = (int)(j / (L.cin * L.ks));
      const int rem = (int)(j - (int64_t)co * L.cin * L.ks);
      ci = rem / L.ks;
      shift = (L.ks - 1 - (rem - ci * L.ks)) * L.dil;
    } else {
      co = (int)(j - nW);
    }
    const int b0 = (int)((int64_t)p.B * seg / 4), b1 = (int)((int64_t)p.B * (seg + 1) / 4);
    double a0 = 0.0, a1 = 0.0;
    for (int b = b0; b < b1; ++b) {
      const float* G = L.g_slot == VQT_SLOT_DPRED ? p.dpred + ((int64_t)b * p.T - 7) * p.nv + co
                                                  : p.act + ((int64_t)b * VQT_SLOTS + L.g_slot) * R * e + co;
      const int gs = L.g_slot == VQT_SLOT_DPRED ? p.nv : e;
      if (!is_w) {
        int r = L.fo;
        for (; r + 1 < R; r += 2) { a0 += G[(int64_t)r * gs]; a1 += G[(int64_t)(r + 1) * gs]; }
        if (r < R) a0 += G[(int64_t)r * gs];
      } else if (L.in_slot == VQT_SLOT_X) {
        const float* X = p.x + ((int64_t)b * p.T - 7) * p.nv + ci;   // rows below 7 are the zero padding: skipped
        int r = L.fo > 7 ? L.fo : 7;
        for (; r + 1 < R; r += 2) {
          a0 += vqt_mul(G[(int64_t)r * gs], X[(int64_t)r * p.nv]);
          a1 += vqt_mul(G[(int64_t)(r + 1) * gs], X[(int64_t)(r + 1) * p.nv]);
        }
        if (r < R) a0 += vqt_mul(G[(int64_t)r * gs], X[(int64_t)r * p.nv]);
      } else {
        const float* In = p.act + ((int64_t)b * VQT_SLOTS + L.in_slot) * R * e + ci - (int64_t)shift * e;
        int r = L.fo;
        for (; r + 1 < R; r += 2) {
          a0 += vqt_mul(G[(int64_t)r * gs], In[(int64_t)r * e]);
          a1 += vqt_mul(G[(int64_t)(r + 1) * gs], In[(int64_t)(r + 1) * e]);
        }
        if (r < R) a0 += vqt_mul(G[(int64_t)r * gs], In[(int64_t)r * e]);
      }
    }
    acc = a0 + a1;
  }
  part[seg][el] = acc;
  __syncthreads();
  if (seg == 0 && idx < p.total) {
    const VqtLayer& L = p.L[li];
    const double s = ((part[0][el] + part[1][el]) + part[2][el]) + part[3][el];
    p.grads[j < nW ? L.w_off + j : L.b_off + (j - nW)] = (float)s;
  }
}

// ---- code statistics: EuclideanCodebook.forward's one-hot sums, then ema_inplace ------------------------------------------
__global__ __launch_bounds__(256) void vqt_stats_kernel(const VqTrainP p) {
  const int gw = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (gw >= p.depth * p.categories) return;  // whole waves leave: no workgroup barrier below
  const int k = gw / p.categories, c = gw - k * p.categories, depth = p.depth, e = p.e;
  const int64_t N = (int64_t)p.B * p.T;
  for (int i0 = 0; i0 < e; i0 += 64) {
    const int i = i0 + lane;
    double sum = 0.0;
    int count = 0;
    for (int64_t base = 0; base < N; base += 64) {
      const int64_t row = base + lane;
      const bool hit = row < N && p.tokens[row * depth + k] == c;
      unsigned long long mask = __ballot(hit);
      count += __popcll(mask);
      while (mask) {  // ascending rows: one order of additions
        const int jrow = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        if (i < e) sum += p.res[((base + jrow) * depth + k) * e + i];
      }
    }
    if (i < e) {
      float* avg = p.embed_avg[k] + (int64_t)c * e + i;
      *avg = *avg * p.decay + (float)sum * p.one_minus_decay;
    }
    if (i0 == 0 && lane == 0) {
      p.rawcount[gw] = (float)count;
      p.cluster[k][c] = p.cluster[k][c] * p.decay + (float)count * p.one_minus_decay;
    }
  }
}

// ---- blocks [0, depth): embed of one level; block depth: the loss record; the rest: AdamW (torch's single-tensor path) --------
__global__ __launch_bounds__(256) void vqt_update_kernel(const VqTrainP p) {
  __shared__ float red[4];
  const int tid = threadIdx.x, depth = p.depth, C = p.categories, e = p.e;
  if ((int)blockIdx.x < depth) {
    const int k = blockIdx.x;
    const float* cs = p.cluster[k];
    float s = 0.f;
    for (int c = tid; c < C; c += 256) s += cs[c];
    const float total = vqt_block_sum(s, red);
    const float den = total + (float)C * p.eps_ema;
    for (int i = tid; i < C * e; i += 256) {
      const float smoothed = (cs[i / e] + p.eps_ema) / den * total;  // laplace_smoothing(cluster_size) * cluster_size.sum()
      p.embed[k][i] = p.embed_avg[k][i] / smoothed;
    }
    return;
  }
  if ((int)blockIdx.x == depth) {
    const int64_t N = (int64_t)p.B * p.T;
    float commit = 0.f;
    for (int k = 0; k < depth; ++k) {
      float s = 0.f;
      for (int64_t r = tid; r < N; r += 256) s += p.rowcommit[r * depth + k];
      commit += vqt_block_sum(s, red) / ((float)N * (float)e);  // F.mse_loss of the level
    }
    commit /= (float)depth;
    float sm_m = 0.f, sm_v = 0.f;
    for (int b = tid; b < p.B; b += 256) { sm_m += p.seqloss[2 * b]; sm_v += p.seqloss[2 * b + 1]; }
    const float motion = vqt_block_sum(sm_m, red) / ((float)N * (float)p.nv);
    const float velsum = vqt_block_sum(sm_v, red);
    const float vel = p.loss_vel > 0.f && p.nv > 1 ? velsum / ((float)N * (float)(p.nv - 1)) : 0.f;
    // compute_perplexity of the last level's tokens: exp(-sum p log(p + 1e-7))
    const float* cnt = p.rawcount + (int64_t)(depth - 1) * C;
    float ent = 0.f;
    for (int c = tid; c < C; c += 256) {
      const float pr = cnt[c] / (float)N;
      ent += pr * logf(pr + 1e-7f);
    }
    ent = vqt_block_sum(ent, red);
    if (tid == 0) {
      float* rec = p.record;
      rec[0] += motion + p.commit * commit + p.loss_vel * vel;
      rec[1] += motion;
      rec[2] += commit;
      rec[3] += vel;
      rec[4] += expf(-ent);
      rec[5] += 1.0f;
    }
    return;
  }
  const int64_t i = ((int64_t)blockIdx.x - depth - 1) * 256 + tid;
  if (i >= p.n_params || (i >= p.pms_off && i < p.pms_off + p.pms_n)) return;  // project_mean_shape never gets a gradient
  const float g = p.grads[i];
  float w = p.params[i];
  w *= 1.0f - p.lr_wd;
  float m = p.m1[i], v = p.m2[i];
  m += (g - m) * 0.1f;                    // exp_avg.lerp_(grad, 1 - beta1), beta1 = 0.9
  v = v * 0.99f + 0.01f * g * g;          // beta2 = 0.99
  const float denom = sqrtf(v) / p.bc2_sqrt + 1e-8f;
  w -= p.step_size * (m / denom);
  p.params[i] = w;
  p.m1[i] = m;
  p.m2[i] = v;
}
