// Decoder layers (audio2photoreal_amd/decoder.py): the convolution every network of the reference's body renderer is made of --
// visualize/ca_body/nn/layers.py Conv2dWNUB (a weight-normalised convolution with an untied bias [C_out, H, W]) inside the
// residual blocks ConvBlock and UpConvBlockDeep of nn/blocks.py -- and the SeamSampler of utils/seams.py.  fp32 like the
// reference.  No atomics; every sum runs in a fixed order inside one thread, so a frame's result depends on neither N nor its
// index and two runs give the same bits.  The weights arrive folded (w = v g / ||v||, decoder.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CONV_MAX_CHANNELS 4096   // C_in / groups and C_out / groups (the loops have no structural limit; this bounds the indices)
#define CONV_MAX_SIZE 16384      // H, W and the source sizes: a plane stays below 2^31 elements
#define CONV_THREADS 256
#define CONV_TW 32               // output tile: 8 rows x 32 columns, one pixel per thread; a wave covers two full rows
#define CONV_TH 8
#define CONV_CI_T 8              // input channels staged in the LDS per step (k = 3)
#define SEAM_THREADS 256
#define SEAM_PLANE_GROUP 8       // planes one thread of seam_resample_kernel writes for its texel

// A source tensor [N, C, Hs, Ws] (frame stride n_stride elements: a channel window of a larger tensor is a source too) read at
// the output's resolution [H, W].  When the sizes differ the read goes through nn.UpsamplingBilinear2d(size = (H, W)), i.e.
// bilinear interpolation with align_corners = True, computed on the fly: the upsampled tensor is never written.
struct ConvSrc {
  const float* p;
  int64_t n_stride;
  int Hs, Ws;
  int up;          // 0: Hs == H and Ws == W, read directly
  float sy, sx;    // (Hs - 1) / (H - 1) and (Ws - 1) / (W - 1) in float32, 0 when the output side is 1
};

struct ConvParams {
  ConvSrc x;                 // main source, C_in = groups * cin_pg channels
  const float* w;            // [C_out, cin_pg, k, k]
  const float* bias;         // bias_mode 1: [C_out]; 2: [C_out, H, W]
  ConvSrc s;                 // skip_mode 2: second source, groups * cs_pg channels
  const float* skip;         // skip_mode 1: [N, C_out, H, W]
  const float* sw;           // skip_mode 2: [C_out, cs_pg]
  const float* sb;           // skip_mode 2: [C_out] or NULL
  const float* mask;         // [H, W] or NULL
  float* out;                // [N, C_out, H, W]
  int C_out, H, W, tiles_x, tiles;   // tiles = tiles_x * tiles_y
  int cin_pg, cout_pg, cs_pg, chunks;   // chunks = ceil(cout_pg / CO_T)
  int bias_mode, act, skip_mode;
  float slope;
};

// One output position of a source: the four taps of the align_corners = True interpolation, as offsets inside a plane, and the
// two fractions.  PyTorch's rule: src = scale * dst in float32, i0 = min((int)src, size - 1), i1 = i0 + (i0 < size - 1),
// lambda = src - i0.  A position outside the output plane (the zero padding of the convolution) has ok = false.
struct ConvTap {
  int o00, o01, o10, o11;
  float ly, lx;
  bool ok;
};

__device__ __forceinline__ ConvTap conv_tap(const ConvSrc& s, int y, int x, int H, int W) {
  ConvTap t;
  t.ok = y >= 0 && y < H && x >= 0 && x < W;
  t.ly = t.lx = 0.0f;
  t.o00 = t.o01 = t.o10 = t.o11 = 0;
  if (!t.ok) return t;
  if (!s.up) {
    t.o00 = y * s.Ws + x;
    return t;
  }
  const float fy = s.sy * (float)y, fx = s.sx * (float)x;
  const int y0 = min((int)fy, s.Hs - 1), x0 = min((int)fx, s.Ws - 1);
  const int y1 = y0 + (y0 < s.Hs - 1 ? 1 : 0), x1 = x0 + (x0 < s.Ws - 1 ? 1 : 0);
  t.ly = fminf(fmaxf(fy - (float)y0, 0.0f), 1.0f);
  t.lx = fminf(fmaxf(fx - (float)x0, 0.0f), 1.0f);
  t.o00 = y0 * s.Ws + x0;
  t.o01 = y0 * s.Ws + x1;
  t.o10 = y1 * s.Ws + x0;
  t.o11 = y1 * s.Ws + x1;
  return t;
}

// The value of one plane at a tap: (1 - ly) ((1 - lx) a00 + lx a01) + ly ((1 - lx) a10 + lx a11), 0 outside the plane.
__device__ __forceinline__ float conv_read(const float* __restrict__ plane, const ConvTap& t, bool up) {
  if (!t.ok) return 0.0f;
  if (!up) return plane[t.o00];
  const float top = (1.0f - t.lx) * plane[t.o00] + t.lx * plane[t.o01];
  const float bot = (1.0f - t.lx) * plane[t.o10] + t.lx * plane[t.o11];
  return (1.0f - t.ly) * top + t.ly * bot;
}

// Direct convolution for few channels, stride 1, zero padding K / 2, with everything a decoder block needs in the same launch:
//   v   = sum over ci (ascending), ky, kx (row-major) of w[oc][ci][ky][kx] x[n][g cin_pg + ci][y + ky - K/2][x + kx - K/2]
//   v   = v + bias          (tied [C_out] or untied [C_out, H, W])
//   v   = v >= 0 ? v : slope v
//   v   = v + skip          (a tensor, or sb[oc] + sum over cs (ascending) of sw[oc][cs] s[n][g cs_pg + cs][y][x])
//   out = v * mask[y][x]
// x and s are read through conv_read, so either may be an upsampled source.
//
// Grid (tiles * N, groups * chunks): block (bx, by) is tile bx % tiles of frame bx / tiles, and chunk by % chunks of group by /
// chunks: CO_T consecutive output channels of one group.  A thread owns one pixel of the 8 x 32 tile and keeps CO_T accumulators
// (plus CO_T for a convolved skip).  K = 3: the input channels of the group pass through the LDS CONV_CI_T at a time as
// (8 + 2) x (32 + 2) halo tiles -- the interpolation of an upsampled source is evaluated once per halo element, not once per
// tap -- and a thread reads its 3 x 3 window from there (consecutive lanes, consecutive words: no bank conflict).  K = 1 reads
// the pixel directly.  The weights are indexed by block and loop counters alone, so they are wave-uniform loads that stay out
// of the vector registers.  LDS 8 x 340 x 4 = 10880 bytes; registers are independent of the channel counts.
template <int K, int CO_T>
__global__ __launch_bounds__(CONV_THREADS) void conv2d_ub_kernel(const ConvParams p) {
  constexpr int R = K / 2, LW = CONV_TW + 2 * R, LH = CONV_TH + 2 * R, LN = LW * LH, KK = K * K;
  constexpr int SLOTS = (LN + CONV_THREADS - 1) / CONV_THREADS;
  __shared__ float tile[K == 3 ? CONV_CI_T * LN : 1];
  const int tid = threadIdx.x, tx = tid % CONV_TW, ty = tid / CONV_TW;
  const int64_t n = blockIdx.x / p.tiles;
  const int bt = blockIdx.x % p.tiles;
  const int y0 = (bt / p.tiles_x) * CONV_TH, x0 = (bt % p.tiles_x) * CONV_TW;
  const int g = blockIdx.y / p.chunks, co0 = (blockIdx.y % p.chunks) * CO_T;
  const int oy = y0 + ty, ox = x0 + tx;
  const bool inside = oy < p.H && ox < p.W;
  const int C_out = p.C_out;

  float acc[CO_T];
#pragma unroll
  for (int co = 0; co < CO_T; ++co) acc[co] = 0.0f;

  const int64_t x_plane = (int64_t)p.x.Hs * p.x.Ws;
  const float* xg = p.x.p + n * p.x.n_stride + (int64_t)g * p.cin_pg * x_plane;     // channel 0 of the group
  const float* wg = p.w + ((int64_t)g * p.cout_pg + co0) * p.cin_pg * KK;           // row co0 of the group

  if (K == 3) {
    ConvTap halo[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int e = tid + s * CONV_THREADS;
      halo[s] = conv_tap(p.x, e < LN ? y0 - R + e / LW : -1, x0 - R + e % LW, p.H, p.W);
    }
    for (int ci0 = 0; ci0 < p.cin_pg; ci0 += CONV_CI_T) {
      const int nci = min(CONV_CI_T, p.cin_pg - ci0);
      __syncthreads();                                        // the previous step's reads are done
      for (int c = 0; c < nci; ++c) {
        const float* plane = xg + (int64_t)(ci0 + c) * x_plane;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
          const int e = tid + s * CONV_THREADS;
          if (e < LN) tile[c * LN + e] = conv_read(plane, halo[s], p.x.up);
        }
      }
      __syncthreads();
      for (int c = 0; c < nci; ++c) {
        float xv[KK];
#pragma unroll
        for (int ky = 0; ky < K; ++ky)
#pragma unroll
          for (int kx = 0; kx < K; ++kx) xv[ky * K + kx] = tile[c * LN + (ty + ky) * LW + tx + kx];
        const float* wc = wg + (int64_t)(ci0 + c) * KK;
#pragma unroll
        for (int co = 0; co < CO_T; ++co) {
          if (co0 + co < p.cout_pg) {                         // wave-uniform
            const float* wr = wc + (int64_t)co * p.cin_pg * KK;
#pragma unroll
            for (int t = 0; t < KK; ++t) acc[co] += wr[t] * xv[t];
          }
        }
      }
    }
  } else {
    ConvTap own = conv_tap(p.x, oy, ox, p.H, p.W);
    for (int ci = 0; ci < p.cin_pg; ++ci) {
      const float xv = conv_read(xg + (int64_t)ci * x_plane, own, p.x.up);
#pragma unroll
      for (int co = 0; co < CO_T; ++co)
        if (co0 + co < p.cout_pg) acc[co] += wg[(int64_t)co * p.cin_pg + ci] * xv;
    }
  }

  float sk[CO_T];
#pragma unroll
  for (int co = 0; co < CO_T; ++co) sk[co] = 0.0f;
  if (p.skip_mode == 2) {
    const ConvTap own = conv_tap(p.s, oy, ox, p.H, p.W);
    const int64_t s_plane = (int64_t)p.s.Hs * p.s.Ws;
    const float* sg = p.s.p + n * p.s.n_stride + (int64_t)g * p.cs_pg * s_plane;
    const float* swg = p.sw + ((int64_t)g * p.cout_pg + co0) * p.cs_pg;
#pragma unroll
    for (int co = 0; co < CO_T; ++co)
      if (p.sb && co0 + co < p.cout_pg) sk[co] = p.sb[g * p.cout_pg + co0 + co];
    for (int cs = 0; cs < p.cs_pg; ++cs) {
      const float sv = conv_read(sg + (int64_t)cs * s_plane, own, p.s.up);
#pragma unroll
      for (int co = 0; co < CO_T; ++co)
        if (co0 + co < p.cout_pg) sk[co] += swg[(int64_t)co * p.cs_pg + cs] * sv;
    }
  }
  if (!inside) return;

  const int64_t HW = (int64_t)p.H * p.W, pix = (int64_t)oy * p.W + ox;
  const float m = p.mask ? p.mask[pix] : 1.0f;
#pragma unroll
  for (int co = 0; co < CO_T; ++co) {
    if (co0 + co >= p.cout_pg) break;
    const int oc = g * p.cout_pg + co0 + co;
    float v = acc[co];
    if (p.bias_mode == 1) v += p.bias[oc];
    if (p.bias_mode == 2) v += p.bias[oc * HW + pix];
    if (p.act) v = v >= 0.0f ? v : p.slope * v;
    if (p.skip_mode == 1) v += p.skip[(n * C_out + oc) * HW + pix];
    if (p.skip_mode == 2) v += sk[co];
    if (p.mask) v *= m;
    p.out[(n * C_out + oc) * HW + pix] = v;
  }
}

// SeamSampler.impaint in two launches over a scratch array [planes, P], so that every source is read from the tensor as it was
// before the call: gather value[plane][src[p]] into scratch, then scatter scratch to value[plane][dst[p]].  dst holds each
// texel at most once (the host keeps the last pair of a repeated destination).  One thread per (plane, pair).
__global__ __launch_bounds__(SEAM_THREADS) void seam_gather_kernel(const float* __restrict__ value, int64_t planes, int64_t HW,
                                                                   const int* __restrict__ src, int P, float* __restrict__ scratch) {
  const int64_t i = (int64_t)blockIdx.x * SEAM_THREADS + threadIdx.x;
  if (i >= planes * P) return;
  scratch[i] = value[(i / P) * HW + src[i % P]];
}

__global__ __launch_bounds__(SEAM_THREADS) void seam_scatter_kernel(float* __restrict__ value, int64_t planes, int64_t HW,
                                                                    const int* __restrict__ dst, int P, const float* __restrict__ scratch) {
  const int64_t i = (int64_t)blockIdx.x * SEAM_THREADS + threadIdx.x;
  if (i >= planes * P) return;
  value[(i / P) * HW + dst[i % P]] = scratch[i];
}

// SeamSampler.resample: out = (1 - w) tex + w grid_sample(tex, 2 (uvs - 0.5), bilinear, align_corners = False, border).
// Grid tblocks * groups (tblocks = ceil(H W / SEAM_THREADS), groups = ceil(planes / SEAM_PLANE_GROUP)).  A thread owns one
// texel: it turns the texel's uv into a pixel position once, by grid_sample's own float32 operations --
//   g = 2 (u - 0.5),  x = ((g + 1) W - 1) / 2 clamped to [0, W - 1],  likewise y with H --
// and for each plane of its group sums the taps nw, ne, sw, se in that order with the weights (xe - x)(ys - y), (x - xw)(ys - y),
// (xe - x)(y - yn), (x - xw)(y - yn), where xw = floor(x), xe = xw + 1, yn = floor(y), ys = yn + 1; a tap outside the plane
// (only ever one with weight 0, at the clamped border) counts 0.
__global__ __launch_bounds__(SEAM_THREADS) void seam_resample_kernel(const float* __restrict__ tex, int64_t planes, int H, int W,
                                                                     const float* __restrict__ uvs, const float* __restrict__ weights,
                                                                     int64_t tblocks, float* __restrict__ out) {
  const int64_t HW = (int64_t)H * W;
  const int64_t t = (blockIdx.x % tblocks) * SEAM_THREADS + threadIdx.x;
  if (t >= HW) return;
  const int64_t p0 = (blockIdx.x / tblocks) * SEAM_PLANE_GROUP, p1 = min(planes, p0 + SEAM_PLANE_GROUP);
  const float gx = 2.0f * (uvs[2 * t] - 0.5f), gy = 2.0f * (uvs[2 * t + 1] - 0.5f);
  const float x = fminf(fmaxf(((gx + 1.0f) * (float)W - 1.0f) / 2.0f, 0.0f), (float)(W - 1));
  const float y = fminf(fmaxf(((gy + 1.0f) * (float)H - 1.0f) / 2.0f, 0.0f), (float)(H - 1));
  const float xw = floorf(x), yn = floorf(y), xe = xw + 1.0f, ys = yn + 1.0f;
  const float w_nw = (xe - x) * (ys - y), w_ne = (x - xw) * (ys - y), w_sw = (xe - x) * (y - yn), w_se = (x - xw) * (y - yn);
  const int ix = (int)xw, iy = (int)yn;
  const bool east = ix + 1 <= W - 1, south = iy + 1 <= H - 1;
  const int o_nw = iy * W + ix, o_ne = o_nw + (east ? 1 : 0), o_sw = o_nw + (south ? W : 0), o_se = o_sw + (east ? 1 : 0);
  const float wt = weights[t];
  for (int64_t pl = p0; pl < p1; ++pl) {
    const float* plane = tex + pl * HW;
    float s = plane[o_nw] * w_nw;
    s += (east ? plane[o_ne] : 0.0f) * w_ne;
    s += (south ? plane[o_sw] : 0.0f) * w_sw;
    s += (east && south ? plane[o_se] : 0.0f) * w_se;
    out[pl * HW + t] = (1.0f - wt) * plane[t] + wt * s;
  }
}
