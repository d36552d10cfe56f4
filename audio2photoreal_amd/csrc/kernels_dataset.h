// Test-split batch assembly (include/a2p_hip.h "capture dataset"; reference data_loaders/data.py:223-253 + tensors.py:71-86):
// z-normalisation of the ground-truth motion and the two-channel audio of B chunks of resident takes, written straight into the
// layouts the models take.  One launch: the first `motion_blocks` workgroups transpose 64-frame x 64-channel motion tiles through
// LDS (rows of the take are read along the channels, `inp` is written along the frames: both sides 256-byte wave accesses), the
// others stream the audio as 16-byte vectors.  Nothing here is reused: the launch is bound by HBM bandwidth (the audio is 97 % of
// its bytes at face B = 8), one pass, no atomics.
//
// Arithmetic is the reference's and nothing else: motion (x - mean) / std in fp64 (numpy promotes the float32 poses against the
// float64 statistics), times the fp64 presence flag for the face (`motion *= missing`, a real product: -x * 0 = -0), rounded ONCE
// to fp32; audio (a - mean[c]) / std in fp32.  Every value is then added to +0.0f, because `collate_tensors` adds each sample
// into a zeroed canvas (tensors.py:23-28): the -0.0 a negative face code leaves on a missing frame becomes +0.0.  IEEE
// subtraction, division and addition only -- this translation unit is built without fast-math, and there is no
// reciprocal-multiply -- so the outputs carry the reference's bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int DS_MAX_BATCH = 64;     // A2P_DATASET_MAX_BATCH
constexpr int DS_TILE = 64;          // motion tile: 64 frames x 64 channels
constexpr int DS_AUDIO_VEC = 4;      // float4 per thread of an audio workgroup (256 threads x 4 x 16 B = 16 KiB per workgroup)

struct DatasetChunk {                // pointers already advanced to the chunk's first frame
  const void* motion;                // [T, C] fp32 | fp64
  const uint8_t* present;            // [T] 1: face frame present, 0: missing; NULL: all present
  const float* audio;                // [T * spf, 2]
  int f64;                           // the motion is fp64
};

struct DatasetP {
  DatasetChunk ch[DS_MAX_BATCH];
  const double* mean;                // [C]
  const double* stdv;                // [C]
  float* inp;                        // [B, C, 1, T]
  float* kf;                         // [B, K, C]
  float* miss;                       // [B, T, C]
  float* audio;                      // [B, T * spf, 2]
  int64_t n4;                        // float4 (= 2 stereo samples) per chunk
  int B, C, T, K, step, face, swap;
  int tiles_c, tiles_t, motion_blocks, audio_bpc;
  float am0, am1, astd;
};

template <bool F64>
__device__ __forceinline__ void dataset_motion_tile(const DatasetP& p, int blk, float (*tile)[DS_TILE + 1]) {
  const int tc = blk % p.tiles_c, tt = (blk / p.tiles_c) % p.tiles_t, b = blk / (p.tiles_c * p.tiles_t);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = tc * DS_TILE, t0 = tt * DS_TILE;
  const DatasetChunk ch = p.ch[b];
  const int c = c0 + lane;
  const bool c_ok = c < p.C;
  const double mean = c_ok ? p.mean[c] : 0.0, sd = c_ok ? p.stdv[c] : 1.0;
  for (int r = wave; r < DS_TILE; r += 4) {      // one wave per frame: 64 consecutive channels
    const int t = t0 + r;
    if (t >= p.T || !c_ok) continue;
    const int64_t at = (int64_t)t * p.C + c;
    const double x = F64 ? static_cast<const double*>(ch.motion)[at] : (double)static_cast<const float*>(ch.motion)[at];
    double v = (x - mean) / sd;
    float present = 1.0f;
    if (p.face) {
      present = (ch.present && ch.present[t] == 0) ? 0.0f : 1.0f;
      v = v * (double)present;
    }
    const float o = (float)v + 0.0f;              // the collate canvas: -0.0 -> +0.0
    tile[r][lane] = o;
    p.miss[((int64_t)b * p.T + t) * p.C + c] = present;
    if (t % p.step == 0) p.kf[((int64_t)b * p.K + t / p.step) * p.C + c] = o;
  }
  __syncthreads();
  for (int r = wave; r < DS_TILE; r += 4) {      // one wave per channel: 64 consecutive frames
    const int cc = c0 + r, t = t0 + lane;
    if (cc < p.C && t < p.T) p.inp[((int64_t)b * p.C + cc) * p.T + t] = tile[lane][r];
  }
}

__device__ __forceinline__ void dataset_audio_part(const DatasetP& p, int blk) {
  const int b = blk / p.audio_bpc, part = blk % p.audio_bpc;
  const float4* src = reinterpret_cast<const float4*>(p.ch[b].audio);
  float4* dst = reinterpret_cast<float4*>(p.audio) + (int64_t)b * p.n4;
  const int64_t base = (int64_t)part * (256 * DS_AUDIO_VEC) + threadIdx.x;
  float4 v[DS_AUDIO_VEC];
#pragma unroll
  for (int j = 0; j < DS_AUDIO_VEC; ++j) {       // all loads in flight before the first division
    const int64_t i = base + j * 256;
    if (i < p.n4) v[j] = src[i];
  }
#pragma unroll
  for (int j = 0; j < DS_AUDIO_VEC; ++j) {
    const int64_t i = base + j * 256;
    if (i >= p.n4) continue;
    float4 a = v[j];
    if (p.swap) a = make_float4(a.y, a.x, a.w, a.z);
    float4 o;
    o.x = (a.x - p.am0) / p.astd + 0.0f;
    o.y = (a.y - p.am1) / p.astd + 0.0f;
    o.z = (a.z - p.am0) / p.astd + 0.0f;
    o.w = (a.w - p.am1) / p.astd + 0.0f;
    dst[i] = o;
  }
}

__global__ __launch_bounds__(256) void dataset_batch_kernel(const DatasetP p) {
  __shared__ float tile[DS_TILE][DS_TILE + 1];
  const int blk = blockIdx.x;
  if (blk < p.motion_blocks) {
    if (p.ch[blk / (p.tiles_c * p.tiles_t)].f64) dataset_motion_tile<true>(p, blk, tile);
    else dataset_motion_tile<false>(p, blk, tile);
  } else {
    dataset_audio_part(p, blk - p.motion_blocks);
  }
}
