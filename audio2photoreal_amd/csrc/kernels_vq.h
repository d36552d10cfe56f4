// Residual-VQ encode (model/vqvae.py:499-506 TemporalVertexCodec.encode, :395-430 TemporalVertexEncoder, :364-379
// ResidualVectorQuantization.encode, :169-195 EuclideanCodebook.quantize): poses -> tokens, the inverse of vq_decode_kernel
// (kernels_guide.h).  It lets sampling condition the guide transformer on known poses (sample/generate.py _replace_keyframes).
#pragma once
#include "a2p_common.h"

struct VqEncodeP {
  const float* poses;          // [B][T][nv], keyframe-rate rows in the normalised space
  const float* codebook[8];    // depth x [categories][e]
  const float* norms[8];       // depth x [categories]: |embed|^2 per code, computed once when the weights are staged
  const float* cw[5];          // enc.0: [e][nv][1], enc.{2,4,6,8}: [e][e][2]
  const float* cb[5];
  int T, depth, categories, e, nv;
  int64_t* tokens;             // nullable [B][T][depth]
  float* latents;              // nullable [B][T][e]: the encoder's output
};

// One workgroup per sequence.  The encoder runs out of two LDS ping-pong buffers of (T + 7) rows, like the decode; then wave w
// quantises rows w, w + 4, ... on its own (no workgroup barrier inside the residual loop): per level every lane scores the codes
// lane, lane + 64, ... and the wave reduces (distance, index) pairs.
__global__ __launch_bounds__(256) void vq_encode_kernel(const VqEncodeP p) {
  extern __shared__ float sm[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int T = p.T, e = p.e, nv = p.nv, R = T + 7;  // 7 zero rows of left padding (receptive field 8)
  float* cur = sm;            // [R][e]
  float* nxt = cur + R * e;   // [R][e]
  const float* x = p.poses + (int64_t)b * T * nv;
  // enc.0 (1x1) + LeakyReLU: a padding row is a zero input, so its output is LeakyReLU(bias), not zero
  for (int i = tid; i < R * e; i += 256) {
    const int r = i / e, co = i - r * e;
    float acc = p.cb[0][co];
    if (r >= 7) {
      const float* w = p.cw[0] + (int64_t)co * nv;
      const float* xr = x + (int64_t)(r - 7) * nv;
      for (int ci = 0; ci < nv; ++ci) acc += w[ci] * xr[ci];
    }
    cur[i] = act_lrelu02(acc);
  }
  __syncthreads();
  const int dil[4] = {1, 2, 3, 1};
  int first = 0;  // rows [first, R) of `cur` are valid
  for (int l = 0; l < 4; ++l) {
    const int nf = first + dil[l];  // a valid (unpadded) k=2 conv shortens the front by its dilation
    for (int i = tid; i < (R - nf) * e; i += 256) {
      const int r = nf + i / e, co = i % e;
      const float* w = p.cw[l + 1] + (int64_t)co * e * 2;
      float acc = p.cb[l + 1][co];
      for (int ci = 0; ci < e; ++ci) acc += w[2 * ci] * cur[(r - dil[l]) * e + ci] + w[2 * ci + 1] * cur[r * e + ci];
      nxt[r * e + co] = l < 3 ? act_lrelu02(acc) : acc;  // no activation after the last conv
    }
    __syncthreads();
    float* t = cur; cur = nxt; nxt = t;
    first = nf;
  }
  // first == 7: rows 7.. of `cur` are the T latents
  if (p.latents) {  // uniform branch: every wave has read its share of `cur` before any wave starts changing rows in place
    for (int i = tid; i < T * e; i += 256) p.latents[(int64_t)b * T * e + i] = cur[7 * e + i];
    __syncthreads();
  }
  if (!p.tokens) return;
  for (int t = wid; t < T; t += 4) {
    float* res = cur + (7 + t) * e;  // the residual, updated in place
    for (int k = 0; k < p.depth; ++k) {
      float xx = 0.f;
      for (int i = lane; i < e; i += 64) xx += res[i] * res[i];
      xx = wave_sum(xx);
      const float* book = p.codebook[k];
      float best = INFINITY;
      int bi = p.categories;  // > every valid index: a lane without a finite distance never wins a tie
      for (int c = lane; c < p.categories; c += 64) {
        const float4* w = reinterpret_cast<const float4*>(book + (int64_t)c * e);
        float dot = 0.f;
        for (int j = 0; j < e / 4; ++j) {
          const float4 a = w[j];
          dot += a.x * res[4 * j] + a.y * res[4 * j + 1] + a.z * res[4 * j + 2] + a.w * res[4 * j + 3];
        }
        // -(|x|^2 - 2 x.embed + |embed|^2) maximised == this minimised; ascending c with `<` keeps the lowest index of a tie
        const float dist = (xx - 2.0f * dot) + p.norms[k][c];
        if (dist < best) { best = dist; bi = c; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
      }
      if (bi >= p.categories) bi = 0;  // every distance non-finite (non-finite input): torch's argmax of NaNs is not pinned either
      if (lane == 0) p.tokens[((int64_t)b * T + t) * p.depth + k] = bi;
      __builtin_amdgcn_wave_barrier();  // every lane has read `res` for this level before it changes
      for (int i = lane; i < e; i += 64) res[i] -= book[(int64_t)bi * e + i];
      __builtin_amdgcn_wave_barrier();
    }
  }
}
