// Texture layers (audio2photoreal_amd/texture.py): what the reference's body renderer runs after ConvDecoder to get the final
// texture -- the 4 x 4 stride-2 convolution and transposed convolution of UNetWB (nn/unet.py) and PoseToShadow (nn/shadow.py),
// la.Conv2dWNUB / la.ConvTranspose2dWNUB(.., 4, 2, 1); F.interpolate(mode = "bilinear", align_corners = False); and the
// arithmetic of AutoEncoder.forward_tex (models/mesh_vae_drivable.py) between its seam steps.  Like kernels_conv.h: fp32, NCHW,
// 64-bit offsets, no atomics, every sum in a fixed order inside one thread, so a frame's bits depend on neither N nor its index.
// The weights arrive folded (texture.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_conv.h"

#define TEX_THREADS 256
#define TEX_ACT_NONE 0
#define TEX_ACT_LRELU 1
#define TEX_ACT_SIGMOID 2

struct TexConvParams {
  const float* x;            // [N, C_in, Hs, Ws], frames n_stride floats apart
  int64_t n_stride;
  const float* w;            // down: [C_out, C_in, 4, 4]; transposed: [C_in, C_out, 4, 4]
  const float* bias;         // bias_mode 1: [C_out]; 2: [C_out, H, W]
  const float* skip;         // transposed only: [N, C_out, H, W] or NULL
  float* out;                // [N, C_out, H, W]
  int C_in, C_out, Hs, Ws, H, W, tiles_x, tiles;
  int bias_mode, act;
  float slope, beta;
};

// SIGMOID: the transposed layer only; the down layer's instances carry neither expf nor the divide.
template <bool SIGMOID>
__device__ __forceinline__ float tex_epilogue(const TexConvParams& p, float v, int oc, int64_t HW, int64_t pix, int64_t frame_oc) {
  if (p.bias_mode == 1) v += p.bias[oc];
  if (p.bias_mode == 2) v += p.bias[oc * HW + pix];
  if (p.act == TEX_ACT_LRELU) v = v >= 0.0f ? v : p.slope * v;
  if (SIGMOID && p.act == TEX_ACT_SIGMOID) v = 1.0f / (1.0f + expf(-(v + p.beta)));
  if (p.skip) v += p.skip[frame_oc * HW + pix];
  return v;
}

// Conv2dWNUB(C_in, C_out, H, W, 4, 2, 1) and an optional LeakyReLU:
//   v = sum over ci ascending, then ky, kx row-major, of w[co][ci][ky][kx] x[n][ci][2 y - 1 + ky][2 x - 1 + kx]   (0 outside)
//   v = v + bias;  v = v >= 0 ? v : slope v
// Grid (tiles * N, chunks).  A block owns a TH x TW tile of output pixels and CO_T * WG output channels, WG = 256 / (TH TW): the
// thread tid is pixel tid % (TH TW) of channel group tid / (TH TW).  TH TW is a multiple of 64, so a wave lies inside one group; the
// group index goes through readfirstlane, which lets the compiler fetch the weights with scalar loads (without it: per-lane
// vector loads of one address).  Two instances: 8 x 32 x 1 group for planes (bound by plane traffic) and 8 x 8 x 4 groups
// for the small planes at the bottom of the UNet (bound by the weight stream: four times fewer blocks read each weight).
// Input channels pass through the LDS CI_T at a time as (2 TH + 2) x (2 TW + 2) halo tiles; the row length is even, so a thread
// reads its 4 x 4 window as eight aligned 8-byte words whose lanes are 8 bytes apart (ds_read_b64, conflict-free).
template <int TH, int TW, int CO_T, int CI_T>
__global__ __launch_bounds__(TEX_THREADS) void conv2d_down_kernel(const TexConvParams p) {
  constexpr int PIX = TH * TW, WG = TEX_THREADS / PIX, LW = 2 * TW + 2, LH = 2 * TH + 2, LN = LW * LH;
  static_assert(PIX % 64 == 0 && TEX_THREADS % PIX == 0, "a wave stays inside one channel group");
  __shared__ __attribute__((aligned(16))) float tile[CI_T * LN];
  const int tid = threadIdx.x, pt = tid % PIX, tx = pt % TW, ty = pt / TW;
  const int wgrp = __builtin_amdgcn_readfirstlane(tid / PIX);   // the same in every lane of a wave: says so to the compiler
  const int64_t n = blockIdx.x / p.tiles;
  const int bt = blockIdx.x % p.tiles;
  const int y0 = (bt / p.tiles_x) * TH, x0 = (bt % p.tiles_x) * TW;
  const int co0 = (blockIdx.y * WG + wgrp) * CO_T;
  const int oy = y0 + ty, ox = x0 + tx;

  float acc[CO_T];
#pragma unroll
  for (int co = 0; co < CO_T; ++co) acc[co] = 0.0f;

  const int64_t x_plane = (int64_t)p.Hs * p.Ws;
  const float* xn = p.x + n * p.n_stride;
  const int iy0 = 2 * y0 - 1, ix0 = 2 * x0 - 1;
  for (int ci0 = 0; ci0 < p.C_in; ci0 += CI_T) {
    const int nci = min(CI_T, p.C_in - ci0);
    __syncthreads();                                          // the previous step's reads are done
    for (int e = tid; e < nci * LN; e += TEX_THREADS) {
      const int c = e / LN, r = e % LN, iy = iy0 + r / LW, ix = ix0 + r % LW;
      const bool ok = iy >= 0 && iy < p.Hs && ix >= 0 && ix < p.Ws;
      tile[e] = ok ? xn[(int64_t)(ci0 + c) * x_plane + (int64_t)iy * p.Ws + ix] : 0.0f;
    }
    __syncthreads();
    for (int c = 0; c < nci; ++c) {
      float xv[16];
#pragma unroll
      for (int ky = 0; ky < 4; ++ky) {
        const float2* row = reinterpret_cast<const float2*>(&tile[c * LN + (2 * ty + ky) * LW + 2 * tx]);
        const float2 a = row[0], b = row[1];
        xv[ky * 4 + 0] = a.x;
        xv[ky * 4 + 1] = a.y;
        xv[ky * 4 + 2] = b.x;
        xv[ky * 4 + 3] = b.y;
      }
#pragma unroll
      for (int co = 0; co < CO_T; ++co) {
        if (co0 + co < p.C_out) {                             // wave-uniform
          const float* wr = p.w + ((int64_t)(co0 + co) * p.C_in + ci0 + c) * 16;
#pragma unroll
          for (int t = 0; t < 16; ++t) acc[co] += wr[t] * xv[t];
        }
      }
    }
  }
  if (oy >= p.H || ox >= p.W) return;
  const int64_t HW = (int64_t)p.H * p.W, pix = (int64_t)oy * p.W + ox;
#pragma unroll
  for (int co = 0; co < CO_T; ++co) {
    if (co0 + co >= p.C_out) break;
    const int oc = co0 + co;
    p.out[(n * p.C_out + oc) * HW + pix] = tex_epilogue<false>(p, acc[co], oc, HW, pix, n * p.C_out + oc);
  }
}

// ConvTranspose2dWNUB(C_in, C_out, 2 Hs, 2 Ws, 4, 2, 1) with its epilogues, as four 2 x 2 stride-1 convolutions, one per parity
// class of the output: with (sy, sx) = (Y / 2, X / 2),
//   even Y: ky = 1 reads row sy, ky = 3 row sy - 1;   odd Y: ky = 0 reads row sy + 1, ky = 2 row sy;   likewise kx and columns
//   v = sum over ci ascending, then the four taps with ky ascending, then kx ascending, of w[ci][co][ky][kx] x[n][ci][row][col]
//   v = v + bias;  v = lrelu(v) or 1 / (1 + expf(-(v + beta)));  v = v + skip
// A source position outside the plane contributes w * 0.  Grid and thread layout as conv2d_down_kernel, with the tile counted
// in SOURCE pixels: a thread owns source pixel (sy, sx), i.e. the 2 x 2 output quad (2 sy.., 2 sx..) of CO_T channels (4 CO_T
// accumulators), and reads its 3 x 3 source window from a (TH + 2) x (TW + 2) halo tile that serves all four classes.  The 16
// CO_T weights of an input channel are contiguous in PyTorch's transposed layout [C_in, C_out, 4, 4].
template <int TH, int TW, int CO_T, int CI_T>
__global__ __launch_bounds__(TEX_THREADS) void conv_transpose2d_kernel(const TexConvParams p) {
  constexpr int PIX = TH * TW, WG = TEX_THREADS / PIX, LW = TW + 2, LH = TH + 2, LN = LW * LH;
  static_assert(PIX % 64 == 0 && TEX_THREADS % PIX == 0, "a wave stays inside one channel group");
  __shared__ float tile[CI_T * LN];
  const int tid = threadIdx.x, pt = tid % PIX, tx = pt % TW, ty = pt / TW;
  const int wgrp = __builtin_amdgcn_readfirstlane(tid / PIX);   // the same in every lane of a wave: says so to the compiler
  const int64_t n = blockIdx.x / p.tiles;
  const int bt = blockIdx.x % p.tiles;
  const int y0 = (bt / p.tiles_x) * TH, x0 = (bt % p.tiles_x) * TW;
  const int co0 = (blockIdx.y * WG + wgrp) * CO_T;
  const int sy = y0 + ty, sx = x0 + tx;

  float acc[CO_T][4];                                         // [co][2 (Y % 2) + (X % 2)]
#pragma unroll
  for (int co = 0; co < CO_T; ++co)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[co][q] = 0.0f;

  const int64_t x_plane = (int64_t)p.Hs * p.Ws;
  const float* xn = p.x + n * p.n_stride;
  for (int ci0 = 0; ci0 < p.C_in; ci0 += CI_T) {
    const int nci = min(CI_T, p.C_in - ci0);
    __syncthreads();
    for (int e = tid; e < nci * LN; e += TEX_THREADS) {
      const int c = e / LN, r = e % LN, iy = y0 - 1 + r / LW, ix = x0 - 1 + r % LW;
      const bool ok = iy >= 0 && iy < p.Hs && ix >= 0 && ix < p.Ws;
      tile[e] = ok ? xn[(int64_t)(ci0 + c) * x_plane + (int64_t)iy * p.Ws + ix] : 0.0f;
    }
    __syncthreads();
    for (int c = 0; c < nci; ++c) {
      float xv[3][3];                                         // [row sy - 1 + a][column sx - 1 + b]
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) xv[a][b] = tile[c * LN + (ty + a) * LW + tx + b];
#pragma unroll
      for (int co = 0; co < CO_T; ++co) {
        if (co0 + co < p.C_out) {                             // wave-uniform
          const float* wr = p.w + ((int64_t)(ci0 + c) * p.C_out + co0 + co) * 16;
#pragma unroll
          for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int px = 0; px < 2; ++px) {
              // parity 0: taps k = 1 (window index 1), k = 3 (index 0); parity 1: k = 0 (index 2), k = 2 (index 1)
              const int ky_a = py ? 0 : 1, ky_b = ky_a + 2, ra = py ? 2 : 1, rb = ra - 1;
              const int kx_a = px ? 0 : 1, kx_b = kx_a + 2, ca = px ? 2 : 1, cb = ca - 1;
              float v = acc[co][2 * py + px];
              v += wr[ky_a * 4 + kx_a] * xv[ra][ca];
              v += wr[ky_a * 4 + kx_b] * xv[ra][cb];
              v += wr[ky_b * 4 + kx_a] * xv[rb][ca];
              v += wr[ky_b * 4 + kx_b] * xv[rb][cb];
              acc[co][2 * py + px] = v;
            }
        }
      }
    }
  }
  if (sy >= p.Hs || sx >= p.Ws) return;
  const int64_t HW = (int64_t)p.H * p.W;
#pragma unroll
  for (int co = 0; co < CO_T; ++co) {
    if (co0 + co >= p.C_out) break;
    const int oc = co0 + co;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t pix = (int64_t)(2 * sy + q / 2) * p.W + 2 * sx + q % 2;
      p.out[(n * p.C_out + oc) * HW + pix] = tex_epilogue<true>(p, acc[co][q], oc, HW, pix, n * p.C_out + oc);
    }
  }
}

// One axis of F.interpolate(mode = "bilinear", align_corners = False), PyTorch's rule in float32:
//   src = max((dst + 0.5) scale - 0.5, 0) with scale = n_in / n_out,  i0 = min((int)src, n_in - 1),  i1 = i0 + (i0 < n_in - 1),
//   l1 = src - i0,  l0 = 1 - l1
struct ResizeAxis {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ ResizeAxis resize_axis(int dst, float scale, int n_in) {
  ResizeAxis a;
  const float src = fmaxf(((float)dst + 0.5f) * scale - 0.5f, 0.0f);
  a.i0 = min((int)src, n_in - 1);
  a.i1 = a.i0 + (a.i0 < n_in - 1 ? 1 : 0);
  a.l1 = src - (float)a.i0;
  a.l0 = 1.0f - a.l1;
  return a;
}

// The value of one plane [.., Ws] at an output position: l0y (l0x a00 + l1x a01) + l1y (l0x a10 + l1x a11).
__device__ __forceinline__ float resize_tap(const float* __restrict__ plane, int Ws, const ResizeAxis& y, const ResizeAxis& x) {
  const float* r0 = plane + (int64_t)y.i0 * Ws;
  const float* r1 = plane + (int64_t)y.i1 * Ws;
  return y.l0 * (x.l0 * r0[x.i0] + x.l1 * r0[x.i1]) + y.l1 * (x.l0 * r1[x.i0] + x.l1 * r1[x.i1]);
}

// x [planes, Hs, Ws] -> out [planes, H, W]; one thread per output element, block blockIdx.x % bpp of plane blockIdx.x / bpp (bpp =
// ceil(H W / 256)), so the index arithmetic inside a plane is 32-bit.
__global__ __launch_bounds__(TEX_THREADS) void resize_bilinear_kernel(const float* __restrict__ x, int Hs, int Ws, int H, int W, float sy,
                                                                      float sx, unsigned bpp, float* __restrict__ out) {
  const int64_t pl = blockIdx.x / bpp;
  const unsigned r = (blockIdx.x % bpp) * TEX_THREADS + threadIdx.x, HW = (unsigned)H * (unsigned)W;
  if (r >= HW) return;
  const int oy = (int)(r / (unsigned)W), ox = (int)(r % (unsigned)W);
  out[pl * HW + r] = resize_tap(x + pl * Hs * Ws, Ws, resize_axis(oy, sy, Hs), resize_axis(ox, sx, Ws));
}

// forward_tex between the seam steps, at the output size [N, C, 2 Sh, 2 Sw]:
//   out[n][c][Y][X] = ((resize(t)[n][c][Y][X] + u[n][4 c + 2 (Y % 2) + (X % 2)][Y / 2][X / 2]) tex_std + tex_mean[c][Y][X]) shadow[n or 0][0][Y][X]
// One thread per (n, c, Y / 2, X / 2), block blockIdx.x % bpp of map blockIdx.x / bpp = n C + c (bpp = ceil(Sh Sw / 256)): it reads
// the four pixel-shuffle channels of u at its texel (consecutive lanes, consecutive words), the 3 x 3 window of t through
// resize_tap, and writes the 2 x 2 quad.
__global__ __launch_bounds__(TEX_THREADS) void texture_compose_kernel(const float* __restrict__ t, const float* __restrict__ u,
                                                                      const float* __restrict__ tex_mean, float tex_std,
                                                                      const float* __restrict__ shadow, int64_t shadow_stride, int C, int Sh,
                                                                      int Sw, unsigned bpp, float* __restrict__ out) {
  const unsigned S = (unsigned)Sh * (unsigned)Sw, r = (blockIdx.x % bpp) * TEX_THREADS + threadIdx.x;
  if (r >= S) return;
  const int64_t nc = blockIdx.x / bpp, n = nc / C;
  const int c = (int)(nc % C), sy = (int)(r / (unsigned)Sw), sx = (int)(r % (unsigned)Sw);
  const int W = 2 * Sw;
  const int64_t HW = 4 * (int64_t)S;
  const float* tp = t + nc * S;
  const float* up = u + (n * 4 * C + 4 * c) * S + r;
  const ResizeAxis ay[2] = {resize_axis(2 * sy, 0.5f, Sh), resize_axis(2 * sy + 1, 0.5f, Sh)};
  const ResizeAxis ax[2] = {resize_axis(2 * sx, 0.5f, Sw), resize_axis(2 * sx + 1, 0.5f, Sw)};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t pix = (int64_t)(2 * sy + q / 2) * W + 2 * sx + q % 2;
    float v = resize_tap(tp, Sw, ay[q / 2], ax[q % 2]) + up[(int64_t)q * S];
    v = v * tex_std + tex_mean[c * HW + pix];
    if (shadow) v *= shadow[n * shadow_stride + pix];
    out[nc * HW + pix] = v;
  }
}
