// Encode layers (audio2photoreal_amd/encoder.py): what the reference runs between the samplers' face codes / body poses and the
// renderer's embeddings -- la.LinearWN for all frames of a chunk, the second half of a ConvDownBlock (nn/blocks.py), the inverse
// of linear blend skinning (LinearBlendSkinning.unskinning and LBSModule.unpose, utils/lbs.py) and the texture conditioning of
// FaceEncoder (models/mesh_vae_drivable.py).  Like kernels_conv.h and kernels_texture.h: fp32, 64-bit offsets, no atomics, every
// sum in a fixed order, so a frame's bits depend on neither N nor its index.  The weights arrive folded (encoder.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_skin.h"
#include "kernels_texture.h"

#define LIN_THREADS 256
#define LIN_OT 32                 // output columns of a block
#define LIN_ROWS 64               // rows (frames) of a block: the reuse dimension of a weight tile
#define LIN_KSLICE 256            // terms of one partial sum (A2P_LINEAR_KSLICE)
#define LIN_KC 128                // terms staged in LDS at a time
#define LIN_LD (LIN_KC + 4)       // LDS row length: 16-byte aligned rows, 16 consecutive rows on 16 distinct 16-byte slots

struct LinearParams {
  const float* x;                 // [N, I], rows ldx floats apart
  const float* w;                 // [O, I]
  const float* bias;              // [O] or NULL
  float* out;                     // [N, O], rows ldo floats apart
  float* part;                    // [S, N, O] when S > 1
  int64_t N, ldx, ldo;
  int I, O, S, act;
  float slope;
};

__device__ __forceinline__ float linear_epilogue(const LinearParams& p, float v, int o) {
  if (p.bias) v += p.bias[o];
  if (p.act) v = v >= 0.0f ? v : p.slope * v;
  return v;
}

// out[n][o] = act(sum_i x[n][i] w[o][i] + bias[o]).  The sum over i is cut into S = ceil(I / 256) slices [256 s, min(I, 256 s +
// 256)), S a function of I alone.  Slice s of element (n, o) is ONE fmaf chain, a = 0, a = fmaf(w[o][i], x[n][i], a) for i
// ascending over the slice.  S = 1: the chain's value goes through the epilogue here.  S > 1: it is stored to part[s][n][o]
// and linear_reduce_kernel adds the slices.
// Grid (ceil(O / 32), S, ceil(N / 64)).  A block owns 32 output columns, one slice and up to 64 rows: every weight of the layer is
// read from memory by exactly one block per 64 rows.  The slice passes through LDS 128 terms at a time: 32 weight rows (VEC = 4,
// 2 or 1 floats per load -- the widest that the alignment of the weight rows allows, chosen on the host from I and the pointer;
// a vector never straddles the end of a row because I is a multiple of VEC) and the rows of x.  Thread tid owns column tid % 32
// and the rows tid / 32 + 8 j, j < 8: it reads its weights as float4 (conflict-free at row length 132) and the x rows as float4
// broadcasts (the 32 lanes of a column group read one address).
template <int VEC>
__global__ __launch_bounds__(LIN_THREADS) void linear_partial_kernel(const LinearParams p) {
  __shared__ __attribute__((aligned(16))) float ws[LIN_OT * LIN_LD];
  __shared__ __attribute__((aligned(16))) float xs[LIN_ROWS * LIN_LD];
  const int tid = threadIdx.x, c = tid % LIN_OT, rg = tid / LIN_OT;
  const int o0 = blockIdx.x * LIN_OT, s = blockIdx.y;
  const int64_t n0 = (int64_t)blockIdx.z * LIN_ROWS;
  const int nrows = (int)min((int64_t)LIN_ROWS, p.N - n0);
  const int ks = s * LIN_KSLICE, ke = min(p.I, ks + LIN_KSLICE);

  float acc[LIN_ROWS / 8];
#pragma unroll
  for (int j = 0; j < LIN_ROWS / 8; ++j) acc[j] = 0.0f;

  for (int kc = ks; kc < ke; kc += LIN_KC) {
    const int kn = min(LIN_KC, ke - kc);
    __syncthreads();                                          // the previous chunk's reads are done
    constexpr int VPR = LIN_KC / VEC;                         // vectors of a staged weight row
    for (int e = tid; e < LIN_OT * VPR; e += LIN_THREADS) {
      const int r = e / VPR, kv = (e % VPR) * VEC, o = o0 + r;
      float v[VEC];
#pragma unroll
      for (int t = 0; t < VEC; ++t) v[t] = 0.0f;
      if (o < p.O && kv < kn) {                               // kn is a multiple of VEC: the vector lies inside the row
        const float* src = p.w + (int64_t)o * p.I + kc + kv;
        if constexpr (VEC == 4) {
          const float4 q = *reinterpret_cast<const float4*>(src);
          v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else if constexpr (VEC == 2) {
          const float2 q = *reinterpret_cast<const float2*>(src);
          v[0] = q.x, v[1] = q.y;
        } else {
          v[0] = src[0];
        }
      }
#pragma unroll
      for (int t = 0; t < VEC; ++t) ws[r * LIN_LD + kv + t] = v[t];
    }
    for (int e = tid; e < nrows * LIN_KC; e += LIN_THREADS) {
      const int r = e / LIN_KC, kk = e % LIN_KC;
      xs[r * LIN_LD + kk] = kk < kn ? p.x[(n0 + r) * p.ldx + kc + kk] : 0.0f;
    }
    __syncthreads();
    const float* wrow = ws + c * LIN_LD;
    int kk = 0;
    for (; kk + 4 <= kn; kk += 4) {
      const float4 w = *reinterpret_cast<const float4*>(wrow + kk);
#pragma unroll
      for (int j = 0; j < LIN_ROWS / 8; ++j) {
        const int r = rg + 8 * j;
        if (r < nrows) {
          const float4 xv = *reinterpret_cast<const float4*>(xs + r * LIN_LD + kk);
          float a = acc[j];
          a = fmaf(w.x, xv.x, a);
          a = fmaf(w.y, xv.y, a);
          a = fmaf(w.z, xv.z, a);
          a = fmaf(w.w, xv.w, a);
          acc[j] = a;
        }
      }
    }
    for (; kk < kn; ++kk) {
      const float w = wrow[kk];
#pragma unroll
      for (int j = 0; j < LIN_ROWS / 8; ++j) {
        const int r = rg + 8 * j;
        if (r < nrows) acc[j] = fmaf(w, xs[r * LIN_LD + kk], acc[j]);
      }
    }
  }

  const int o = o0 + c;
  if (o >= p.O) return;
#pragma unroll
  for (int j = 0; j < LIN_ROWS / 8; ++j) {
    const int r = rg + 8 * j;
    if (r >= nrows) continue;
    if (p.S == 1) p.out[(n0 + r) * p.ldo + o] = linear_epilogue(p, acc[j], o);
    else p.part[((int64_t)s * p.N + n0 + r) * p.O + o] = acc[j];
  }
}

// S > 1: v = part[0][n][o]; v = v + part[s][n][o] for s = 1 .. S - 1 ascending; v = v + bias[o]; v = v >= 0 ? v : slope v.
// One thread per (n, o), consecutive lanes on consecutive columns.
__global__ __launch_bounds__(LIN_THREADS) void linear_reduce_kernel(const LinearParams p) {
  const int64_t e = (int64_t)blockIdx.x * LIN_THREADS + threadIdx.x, NO = p.N * p.O;
  if (e >= NO) return;
  const int64_t n = e / p.O;
  const int o = (int)(e % p.O);
  float v = p.part[e];
  for (int s = 1; s < p.S; ++s) v += p.part[(int64_t)s * NO + e];
  p.out[n * p.ldo + o] = linear_epilogue(p, v, o);
}

struct Down3Params {
  const float* h;            // [N, C_in, Hs, Ws], frames h_stride floats apart: lrelu(conv1(x) + b1)
  const float* x;            // [N, C_in, Hs, Ws], frames x_stride floats apart: the block's input
  int64_t h_stride, x_stride;
  const float* w2;           // [C_out, C_in, 3, 3]
  const float* b2;           // [C_out, H, W]
  const float* wr;           // [C_out, C_in]
  const float* br;           // [C_out] or NULL
  float* out;                // [N, C_out, H, W]
  int C_in, C_out, Hs, Ws, H, W, tiles_x, tiles;
  float slope;
};

// The second launch of a ConvDownBlock: lrelu2(conv2(h)) + conv_resize(x), conv2 = Conv2dWNUB(C_in, C_out, 3, stride 2, padding
// 1) and conv_resize = Conv2dWN(C_in, C_out, 1, stride 2).  Per output element, in this order:
//   v = sum over ci ascending, then ky, kx row-major, of w2[co][ci][ky][kx] h[n][ci][2 y - 1 + ky][2 x - 1 + kx]   (0 outside)
//   v = v + b2[co][y][x];  v = v >= 0 ? v : slope v
//   r = sum over ci ascending of wr[co][ci] x[n][ci][2 y][2 x];  v = v + (br[co] + r)          (br NULL counts 0)
// Grid, thread layout and the two tile instances are conv2d_down_kernel's (kernels_texture.h): a block owns a TH x TW tile of
// output pixels and CO_T * WG output channels; the input channels of h pass through LDS CI_T at a time as (2 TH + 1) x (2 TW + 1)
// halo tiles (stored with an even row length); the weights are wave-uniform scalar loads.  x is read at its strided positions
// directly; the 1 x 1 branch is never written to memory.
template <int TH, int TW, int CO_T, int CI_T>
__global__ __launch_bounds__(TEX_THREADS) void conv2d_down3_kernel(const Down3Params p) {
  constexpr int PIX = TH * TW, WG = TEX_THREADS / PIX, LW = 2 * TW + 2, LH = 2 * TH + 1, LN = LW * LH;
  static_assert(PIX % 64 == 0 && TEX_THREADS % PIX == 0, "a wave stays inside one channel group");
  __shared__ float tile[CI_T * LN];
  const int tid = threadIdx.x, pt = tid % PIX, tx = pt % TW, ty = pt / TW;
  const int wgrp = __builtin_amdgcn_readfirstlane(tid / PIX);   // the same in every lane of a wave: says so to the compiler
  const int64_t n = blockIdx.x / p.tiles;
  const int bt = blockIdx.x % p.tiles;
  const int y0 = (bt / p.tiles_x) * TH, x0 = (bt % p.tiles_x) * TW;
  const int co0 = (blockIdx.y * WG + wgrp) * CO_T;
  const int oy = y0 + ty, ox = x0 + tx;
  const bool inside = oy < p.H && ox < p.W;

  float acc[CO_T], res[CO_T];
#pragma unroll
  for (int co = 0; co < CO_T; ++co) acc[co] = res[co] = 0.0f;

  const int64_t plane = (int64_t)p.Hs * p.Ws;
  const float* hn = p.h + n * p.h_stride;
  const float* xn = p.x + n * p.x_stride + (inside ? (int64_t)(2 * oy) * p.Ws + 2 * ox : 0);   // 2 (H - 1) <= Hs - 1: in the plane
  const int iy0 = 2 * y0 - 1, ix0 = 2 * x0 - 1;
  for (int ci0 = 0; ci0 < p.C_in; ci0 += CI_T) {
    const int nci = min(CI_T, p.C_in - ci0);
    __syncthreads();                                          // the previous step's reads are done
    for (int e = tid; e < nci * LN; e += TEX_THREADS) {
      const int c = e / LN, r = e % LN, iy = iy0 + r / LW, ix = ix0 + r % LW;
      const bool ok = iy >= 0 && iy < p.Hs && ix >= 0 && ix < p.Ws;
      tile[e] = ok ? hn[(int64_t)(ci0 + c) * plane + (int64_t)iy * p.Ws + ix] : 0.0f;
    }
    __syncthreads();
    for (int c = 0; c < nci; ++c) {
      float hv[9];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) hv[ky * 3 + kx] = tile[c * LN + (2 * ty + ky) * LW + 2 * tx + kx];
      const float xv = inside ? xn[(int64_t)(ci0 + c) * plane] : 0.0f;
#pragma unroll
      for (int co = 0; co < CO_T; ++co) {
        if (co0 + co < p.C_out) {                             // wave-uniform
          const float* wk = p.w2 + ((int64_t)(co0 + co) * p.C_in + ci0 + c) * 9;
#pragma unroll
          for (int t = 0; t < 9; ++t) acc[co] += wk[t] * hv[t];
          res[co] += p.wr[(int64_t)(co0 + co) * p.C_in + ci0 + c] * xv;
        }
      }
    }
  }
  if (!inside) return;
  const int64_t HW = (int64_t)p.H * p.W, pix = (int64_t)oy * p.W + ox;
#pragma unroll
  for (int co = 0; co < CO_T; ++co) {
    if (co0 + co >= p.C_out) break;
    const int oc = co0 + co;
    float v = acc[co] + p.b2[oc * HW + pix];
    v = v >= 0.0f ? v : p.slope * v;
    p.out[(n * p.C_out + oc) * HW + pix] = v + ((p.br ? p.br[oc] : 0.0f) + res[co]);
  }
}

// LinearBlendSkinning.unskinning and LBSModule.unpose.  Grid, LDS and thread layout are skin_vertices_kernel's (kernels_skin.h).
// Per frame n and vertex v, with g = (gx, gy, gz):
//   M = 0;  M = M + w[k][v] mats[n][idx[k][v]] for k ascending, entry by entry (3 x 4);  A = M[:, 0:3], t = M[:, 3]
//   p = verts[n][v] / g;  d = p - t                                                   (a division, as the reference writes it)
//   C[i][j] = the cofactors of A (adj = C^T), each a difference of two products;  det = A00 C00 + A01 C01 + A02 C02, summed
//   left to right;  u_i = adj[i][0] d_0 + adj[i][1] d_1 + adj[i][2] d_2, left to right
//   out[n][v][i] = u_i / det - template[v][i]
// The reference inverts the 4 x 4 matrix by LU (Tensor.inverse); this is the closed form.  det = 0 or a non-finite det gives a
// non-finite output; nothing is checked here.
__global__ __launch_bounds__(SKIN_THREADS) void unskin_vertices_kernel(
    const float* __restrict__ mats, int J, const float* __restrict__ verts, const float* __restrict__ tmpl,
    const int* __restrict__ idx, const float* __restrict__ w, int V, int K, int tiles, float gx, float gy, float gz,
    float* __restrict__ out) {
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
      float a[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) a[i] = 0.0f;
      for (int k = 0; k < K; ++k) {
        const int j = idx[(int64_t)k * V + v];
        const float wk = w[(int64_t)k * V + v];
        const float* mj = m + 12 * j;
#pragma unroll
        for (int i = 0; i < 12; ++i) a[i] += wk * mj[i];
      }
      const float* pv = verts + (n * V + v) * 3;
      const float d0 = pv[0] / gx - a[3], d1 = pv[1] / gy - a[7], d2 = pv[2] / gz - a[11];
      const float c00 = a[5] * a[10] - a[6] * a[9], c01 = a[6] * a[8] - a[4] * a[10], c02 = a[4] * a[9] - a[5] * a[8];
      const float c10 = a[2] * a[9] - a[1] * a[10], c11 = a[0] * a[10] - a[2] * a[8], c12 = a[1] * a[8] - a[0] * a[9];
      const float c20 = a[1] * a[6] - a[2] * a[5], c21 = a[2] * a[4] - a[0] * a[6], c22 = a[0] * a[5] - a[1] * a[4];
      const float det = a[0] * c00 + a[1] * c01 + a[2] * c02;
      const float* tv = tmpl + 3 * (int64_t)v;
      tile[3 * tid] = (c00 * d0 + c10 * d1 + c20 * d2) / det - tv[0];
      tile[3 * tid + 1] = (c01 * d0 + c11 * d1 + c21 * d2) / det - tv[1];
      tile[3 * tid + 2] = (c02 * d0 + c12 * d1 + c22 * d2) / det - tv[2];
    }
    __syncthreads();
    const int cnt = min(SKIN_THREADS, V - v0) * 3;
    float* o = out + (n * V + v0) * 3;
    for (int i = tid; i < cnt; i += SKIN_THREADS) o[i] = tile[i];
    __syncthreads();
  }
}

// FaceEncoder's texture conditioning in one launch:
//   f(a) = 255 ((raw[n][c][a] + bias[c][a]) + 0.5)                                     face_tex at one source texel
//   r = l0y (l0x f(a00) + l1x f(a01)) + l1y (l0x f(a10) + l1x f(a11))                  a2p_resize_bilinear's taps and weights
//   out[n][c][y][x] = (r / 255 - 0.5) mask[y][x]
// One thread per output element, block blockIdx.x % bpp of plane blockIdx.x / bpp = n C + c as in resize_bilinear_kernel.
__global__ __launch_bounds__(TEX_THREADS) void face_tex_cond_kernel(const float* __restrict__ raw, const float* __restrict__ bias,
                                                                    const float* __restrict__ mask, int C, int Hs, int Ws, int H, int W,
                                                                    float sy, float sx, unsigned bpp, float* __restrict__ out) {
  const int64_t pl = blockIdx.x / bpp;
  const unsigned r = (blockIdx.x % bpp) * TEX_THREADS + threadIdx.x, HW = (unsigned)H * (unsigned)W;
  if (r >= HW) return;
  const int oy = (int)(r / (unsigned)W), ox = (int)(r % (unsigned)W);
  const ResizeAxis y = resize_axis(oy, sy, Hs), x = resize_axis(ox, sx, Ws);
  const float* rp = raw + pl * Hs * Ws;
  const float* bp = bias + (pl % C) * Hs * Ws;
  const int64_t r0 = (int64_t)y.i0 * Ws, r1 = (int64_t)y.i1 * Ws;
  const float f00 = 255.0f * ((rp[r0 + x.i0] + bp[r0 + x.i0]) + 0.5f), f01 = 255.0f * ((rp[r0 + x.i1] + bp[r0 + x.i1]) + 0.5f);
  const float f10 = 255.0f * ((rp[r1 + x.i0] + bp[r1 + x.i0]) + 0.5f), f11 = 255.0f * ((rp[r1 + x.i1] + bp[r1 + x.i1]) + 0.5f);
  const float v = y.l0 * (x.l0 * f00 + x.l1 * f01) + y.l1 * (x.l0 * f10 + x.l1 * f11);
  out[pl * HW + r] = (v / 255.0f - 0.5f) * mask[r];
}
