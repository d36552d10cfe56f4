// Waveform kernels of the recording -> y["audio"] path (audio2photoreal_amd/audio.py, sample/recording.py; the demo's
// generate_results, demo/demo.py:156-189): the rational-ratio windowed-sinc resampler of torchaudio.functional.resample
// (optionally averaging interleaved channels to mono on the way in), and the dual-audio assembly (peak normalisation, partner
// noise channel, z-normalisation, tiling over the repetitions).
#pragma once
#include "a2p_common.h"

// Sample i of row b, channels averaged: C = 2 is (a + b) * 0.5f, the bits torch.mean gives for two float32 values; C > 2 sums in
// channel order and divides by C.
__device__ __forceinline__ float mono_sample(const float* __restrict__ in, int64_t row, int64_t i, int C) {
  const float* p = in + (row + i) * C;
  if (C == 1) return p[0];
  if (C == 2) return (p[0] + p[1]) * 0.5f;
  float s = p[0];
  for (int c = 1; c < C; ++c) s += p[c];
  return s / (float)C;
}

// out[b][m] = sum_j K[m mod n][j] * xpad[(m div n) * o + j], xpad = x with `width` zeros on the left (and width + o on the right):
// torchaudio's conv1d(pad(x, (width, width + o)), kernel, stride=o) with the output phases interleaved.  Taps that fall on the
// padding are skipped (their products are exact zeros), so only real input samples are read.  K == nullptr: equal rates, the
// (downmixed) input is copied.  One thread per output sample, grid-stride.
__global__ void __launch_bounds__(256) resample_sinc_kernel(const float* __restrict__ in, int64_t len, int C, int o, int n,
                                                            const float* __restrict__ K, int taps, int width, int64_t out_len,
                                                            int64_t total, float* __restrict__ out) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = g / out_len, m = g - b * out_len;
    const int64_t row = b * len;
    if (K == nullptr) {
      out[g] = mono_sample(in, row, m, C);
      continue;
    }
    const int64_t q = m / n;
    const int p = (int)(m - q * n);
    const int64_t start = q * o - width;                       // input index under tap 0
    const int j0 = start < 0 ? (int)(-start) : 0;
    const int64_t jend = len - start;
    const int j1 = jend < taps ? (int)jend : taps;
    const float* __restrict__ k = K + (int64_t)p * taps;
    float acc = 0.f;
    for (int j = j0; j < j1; ++j) acc = fmaf(k[j], mono_sample(in, row, start + j, C), acc);
    out[g] = acc;
  }
}

// Dual-audio assembly, step 1 of 2: block maxima of mono[0, len) into partial[blockIdx.x].  NaN propagates (torch's max does).
constexpr int kPeakPartials = 256;
__device__ __forceinline__ float max_nan(float a, float b) { return (b > a || b != b) ? b : a; }

__global__ void __launch_bounds__(256) peak_partial_kernel(const float* __restrict__ mono, int64_t len, float* __restrict__ partial) {
  __shared__ float red[256];
  float m = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x) m = max_nan(m, mono[i]);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = max_nan(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// ... and the maximum of the kPeakPartials partials into partial[kPeakPartials] (one block of kPeakPartials threads).
__global__ void __launch_bounds__(kPeakPartials) peak_final_kernel(float* __restrict__ partial) {
  __shared__ float red[kPeakPartials];
  red[threadIdx.x] = partial[threadIdx.x];
  __syncthreads();
  for (int s = kPeakPartials / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = max_nan(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[kPeakPartials] = red[0];
}

// Step 2: the demo's float64 numpy arithmetic followed by torch.Tensor(...).float():
//   ch0 = float32(((double)(mono[i] / peak) - mean0) / std)     (mono / peak is a float32 division, as torch does it)
//   ch1 = float32((noise[i][1] - mean1) / std)                   (noise: the caller's float64 [len, 2] normal draws)
// written to out[r][i][:] for every repetition r < reps.
__global__ void __launch_bounds__(256) dual_audio_kernel(const float* __restrict__ mono, int64_t len, float peak,
                                                         const double* __restrict__ noise, double mean0, double mean1, double std,
                                                         int reps, float2* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x) {
    const float y = mono[i] / peak;
    const double a = ((double)y - mean0) / std;
    const double b = (noise[2 * i + 1] - mean1) / std;
    const float2 v = make_float2((float)a, (float)b);
    for (int r = 0; r < reps; ++r) out[(int64_t)r * len + i] = v;
  }
}

// ---- conversations: both channels of a two-person recording (sample/conversation.py) ----------------------------------------

// Per-channel resampling: in [len, C] interleaved -> out[c][m] (planar [C, out_len]), channel c alone.  The taps, their order and
// the fmaf chain are resample_sinc_kernel's with C = 1, so row c is bit-identical to that kernel run on channel c extracted as a
// mono row.  K == nullptr: equal rates, the channel is copied.  One thread per output sample, grid-stride.
__global__ void __launch_bounds__(256) resample_channels_kernel(const float* __restrict__ in, int64_t len, int C, int o, int n,
                                                                const float* __restrict__ K, int taps, int width, int64_t out_len,
                                                                int64_t total, float* __restrict__ out) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = g / out_len, m = g - c * out_len;
    const float* __restrict__ x = in + c;                      // sample i of channel c is x[i * C]
    if (K == nullptr) {
      out[g] = x[m * C];
      continue;
    }
    const int64_t q = m / n;
    const int p = (int)(m - q * n);
    const int64_t start = q * o - width;
    const int j0 = start < 0 ? (int)(-start) : 0;
    const int64_t jend = len - start;
    const int j1 = jend < taps ? (int)jend : taps;
    const float* __restrict__ k = K + (int64_t)p * taps;
    float acc = 0.f;
    for (int j = j0; j < j1; ++j) acc = fmaf(k[j], x[(start + j) * C], acc);
    out[g] = acc;
  }
}

// Maxima of both rows of a planar [2, ld] signal over [0, len) in one pass: block maxima into partial[c * kPeakPartials +
// blockIdx.x] (fixed-order tree, as peak_partial_kernel; NaN propagates) ...
__global__ void __launch_bounds__(256) peak2_partial_kernel(const float* __restrict__ x, int64_t ld, int64_t len,
                                                            float* __restrict__ partial) {
  __shared__ float red[2][256];
  float m0 = -INFINITY, m1 = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x) {
    m0 = max_nan(m0, x[i]);
    m1 = max_nan(m1, x[ld + i]);
  }
  red[0][threadIdx.x] = m0;
  red[1][threadIdx.x] = m1;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] = max_nan(red[0][threadIdx.x], red[0][threadIdx.x + s]);
      red[1][threadIdx.x] = max_nan(red[1][threadIdx.x], red[1][threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = red[0][0];
    partial[kPeakPartials + blockIdx.x] = red[1][0];
  }
}

// ... and the two maxima of the partials into partial[2 * kPeakPartials + c] (one block of kPeakPartials threads).
__global__ void __launch_bounds__(kPeakPartials) peak2_final_kernel(float* __restrict__ partial) {
  __shared__ float red[2][kPeakPartials];
  red[0][threadIdx.x] = partial[threadIdx.x];
  red[1][threadIdx.x] = partial[kPeakPartials + threadIdx.x];
  __syncthreads();
  for (int s = kPeakPartials / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] = max_nan(red[0][threadIdx.x], red[0][threadIdx.x + s]);
      red[1][threadIdx.x] = max_nan(red[1][threadIdx.x], red[1][threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[2 * kPeakPartials] = red[0][0];
    partial[2 * kPeakPartials + 1] = red[1][0];
  }
}

// Conversation assembly from the planar channels x [2, ld] (channel k: person k's microphone), for the people in the bitmask
// `people` (bit p: person p):
//   u_k = x[k][i] / peak_k (float32 division) when peaks are given (peak0 > 0), else x[k][i]
//   out[p * reps + r][i] = (float32((u_p - m0_p) / s_p), float32((u_{1-p} - m1_p) / s_p))      (arithmetic in float64)
// for every repetition r < reps.  Rows of a person outside `people` are not written.
__global__ void __launch_bounds__(256) conversation_audio_kernel(const float* __restrict__ x, int64_t ld, int64_t len, float peak0,
                                                                 float peak1, int people, double m00, double m01, double s0, double m10,
                                                                 double m11, double s1, int reps, float2* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x) {
    float u0 = x[i], u1 = x[ld + i];
    if (peak0 > 0.f) {
      u0 = u0 / peak0;
      u1 = u1 / peak1;
    }
    if (people & 1) {
      const float2 v = make_float2((float)(((double)u0 - m00) / s0), (float)(((double)u1 - m01) / s0));
      for (int r = 0; r < reps; ++r) out[(int64_t)r * len + i] = v;
    }
    if (people & 2) {
      const float2 v = make_float2((float)(((double)u1 - m10) / s1), (float)(((double)u0 - m11) / s1));
      for (int r = 0; r < reps; ++r) out[(int64_t)(reps + r) * len + i] = v;
    }
  }
}
