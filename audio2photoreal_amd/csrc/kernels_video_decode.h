// Baseline JPEG back to pixels on the GPU (include/a2p_hip.h "reading video frames"; host wrappers in a2p_video.h; audio2photoreal_amd/
// video.py), the mirror of kernels_video.h:
// jpeg_restarts_kernel  the entropy-coded segment of every frame -> the byte range of every restart interval; a workgroup per frame
//                       scans chunks of 4096 bytes: classify, prefix sum within the workgroup, write positions;
// jpeg_decode_kernel    those intervals -> coefficients in scan order, a lane per restart interval (jpeg_decode_core.h: byte
//                       unstuffing, Huffman lookup from tables in LDS, amplitude extension, DC prediction from 0 in every interval).
//                       Ri = 0 is one interval, and therefore one lane, per frame: slow and correct;
// jpeg_pixels_kernel    coefficients -> uint8 RGB (dequantisation, 8 x 8 inverse DCT, chroma replication, colour transform), fp32
//                       with a fixed fmaf order.
// Integer atomics only (a minimum, independent of the order); a frame's result depends on that frame alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "jpeg_decode_core.h"

#define JPEG_SCAN_CHUNK 4096       // bytes of a segment one pass of jpeg_restarts_kernel classifies: 16 per thread
#define JPEG_DEC_STRIP_PX 128      // luminance pixels of an MCU row one workgroup of jpeg_pixels_kernel owns
#define JPEG_DEC_PSTRIDE 132       // floats between rows of its LDS planes

struct JpegRestartParams {
  const uint8_t* data;
  int64_t data_bytes;
  const int64_t* segments;         // [N][2]: begin and end of every frame's entropy-coded segment in data
  int64_t intervals;
  int64_t* ranges;                 // [N][intervals + 1]
  int32_t* status;                 // [N]
};

// keeps the smallest non-zero status
__device__ __forceinline__ void jpeg_status_min(uint32_t* at, uint32_t v) {
  uint32_t old = *at;
  while (old == 0 || v < old) {
    const uint32_t seen = atomicCAS(at, old, v);
    if (seen == old) break;
    old = seen;
  }
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_restarts_kernel(JpegRestartParams p) {
  __shared__ uint8_t s_bytes[JPEG_SCAN_CHUNK + 4];
  __shared__ int s_wave[JPEG_THREADS / JPEG_WAVE];
  __shared__ uint32_t s_status;
  const int tid = threadIdx.x, lane = tid & (JPEG_WAVE - 1), wave = tid / JPEG_WAVE;
  const int64_t n = blockIdx.x;
  int64_t begin = p.segments[2 * n], end = p.segments[2 * n + 1];
  begin = begin < 0 ? 0 : (begin > p.data_bytes ? p.data_bytes : begin);    // the offsets are input too
  end = end < begin ? begin : (end > p.data_bytes ? p.data_bytes : end);
  int64_t* ranges = p.ranges + n * (p.intervals + 1);
  if (tid == 0) s_status = 0, ranges[0] = begin, ranges[p.intervals] = end;
  constexpr int PER = JPEG_SCAN_CHUNK / JPEG_THREADS;
  int64_t count = 0;                                             // RSTm in front of this chunk
  for (int64_t c0 = begin; c0 < end; c0 += JPEG_SCAN_CHUNK) {
    const int nb = end - c0 < JPEG_SCAN_CHUNK ? (int)(end - c0) : JPEG_SCAN_CHUNK;
    const int have = end - c0 < JPEG_SCAN_CHUNK + 1 ? (int)(end - c0) : JPEG_SCAN_CHUNK + 1;   // one byte of the next chunk: a marker's second
    __syncthreads();
    for (int i = tid; i < have; i += JPEG_THREADS) s_bytes[i] = p.data[c0 + i];
    __syncthreads();
    const int b0 = tid * PER < nb ? tid * PER : nb, b1 = b0 + PER < nb ? b0 + PER : nb;
    int mine = 0;
    for (int i = b0; i < b1; ++i) mine += jpeg_classify(s_bytes, i, have) >= 0;
    const int incl = jpeg_wave_scan(mine, lane);
    if (lane == JPEG_WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    int before = incl - mine, total = 0;
    for (int w = 0; w < JPEG_THREADS / JPEG_WAVE; ++w) {
      if (w < wave) before += s_wave[w];
      total += s_wave[w];
    }
    int64_t k = count + before;
    for (int i = b0; i < b1; ++i) {
      const int kind = jpeg_classify(s_bytes, i, have);
      const int32_t v = jpeg_restart_verdict(kind, k, p.intervals);
      if (v) jpeg_status_min(&s_status, (uint32_t)v);
      if (kind >= 0) {
        if (k + 1 < p.intervals) ranges[k + 1] = c0 + i + 2;
        ++k;
      }
    }
    count += total;
  }
  __syncthreads();
  if (tid == 0) {
    const int64_t last = p.intervals - 1;
    p.status[n] = s_status ? (int32_t)s_status : (count == last ? 0 : JPEG_STATUS(count < last ? count : last, JPEG_ERR_RST_COUNT));
  }
}

struct JpegDecodeParams {
  const uint8_t* data;
  int64_t data_bytes;
  const int64_t* ranges;           // [N][intervals + 1] of jpeg_restarts_kernel
  const int32_t* restart_status;   // [N] or NULL: frames whose scan failed are left alone
  const int32_t* tables;           // [JPEG_TABLES][JPEG_TABLE_WORDS]
  int16_t* coef;                   // [N][mcus][bpm][64], zero
  int32_t* status;                 // [N], zero
  int64_t N, intervals, mcus, ri;  // ri: MCUs of an interval (mcus when the file has no DRI)
  JpegScan scan;
};

__global__ __launch_bounds__(JPEG_WAVE) void jpeg_decode_kernel(JpegDecodeParams p) {
  __shared__ int32_t s_tab[JPEG_TABLES * JPEG_TABLE_WORDS];
  for (int i = threadIdx.x; i < JPEG_TABLES * JPEG_TABLE_WORDS; i += JPEG_WAVE) s_tab[i] = p.tables[i];
  __syncthreads();
  const int64_t g = (int64_t)blockIdx.x * JPEG_WAVE + threadIdx.x;
  if (g >= p.N * p.intervals) return;
  const int64_t n = g / p.intervals, iv = g - n * p.intervals;
  if (p.restart_status && p.restart_status[n]) return;
  const int64_t* ranges = p.ranges + n * (p.intervals + 1);
  int64_t begin = ranges[iv], end = ranges[iv + 1] - (iv + 1 < p.intervals ? 2 : 0);
  begin = begin < 0 ? 0 : (begin > p.data_bytes ? p.data_bytes : begin);    // the ranges are input too
  end = end < begin ? begin : (end > p.data_bytes ? p.data_bytes : end);
  const int64_t m0 = iv * p.ri, m1 = m0 + p.ri < p.mcus ? m0 + p.ri : p.mcus;   // intervals = ceil(mcus / ri): m0 < mcus
  const int cause = jpeg_decode_interval(p.data, begin, end, s_tab, p.scan, m0, m1, p.coef + n * p.mcus * p.scan.bpm * 64);
  if (cause) jpeg_status_min((uint32_t*)p.status + n, (uint32_t)JPEG_STATUS(iv, cause));
}

// ------------------------------------------------------------------------------------------------ pixels
struct JpegPixelParams {
  const int16_t* coef;             // [N, mcu_rows, mcu_cols, bpm, 64]
  const uint16_t* qtab;            // [components][64] in scan order
  uint8_t* out;
  int64_t frame_stride, row_stride;   // bytes
  int H, W, mcu_rows, mcu_cols, strips;
};

// out[x] = sum over u ascending of in[u] c[u][x], the transpose of jpeg_dct8's sum with the same constants
__device__ __forceinline__ void jpeg_idct8(const float (&in)[8], float (&out)[8]) {
  constexpr float c[8][8] = {
      {0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f},
      {0.490392625f, 0.415734798f, 0.277785122f, 0.0975451618f, -0.0975451618f, -0.277785122f, -0.415734798f, -0.490392625f},
      {0.461939752f, 0.191341713f, -0.191341713f, -0.461939752f, -0.461939752f, -0.191341713f, 0.191341713f, 0.461939752f},
      {0.415734798f, -0.0975451618f, -0.490392625f, -0.277785122f, 0.277785122f, 0.490392625f, 0.0975451618f, -0.415734798f},
      {0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f, 0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f},
      {0.277785122f, -0.490392625f, 0.0975451618f, 0.415734798f, -0.415734798f, -0.0975451618f, 0.490392625f, -0.277785122f},
      {0.191341713f, -0.461939752f, 0.461939752f, -0.191341713f, -0.191341713f, 0.461939752f, -0.461939752f, 0.191341713f},
      {0.0975451618f, -0.277785122f, 0.415734798f, -0.490392625f, 0.490392625f, -0.415734798f, 0.277785122f, -0.0975451618f}};
#pragma unroll
  for (int x = 0; x < 8; ++x) {
    float a = in[0] * c[0][x];
#pragma unroll
    for (int u = 1; u < 8; ++u) a = fmaf(in[u], c[u][x], a);
    out[x] = a;
  }
}

// One workgroup per strip of 128 luminance pixels of one MCU row.  HS x VS: the luminance blocks of an MCU (1 x 1, 2 x 1, 2 x 2) over
// one block each of Cb and Cr; GRAY: one component, an MCU is one block.  Phases, each closed by a barrier: the strip's coefficients to
// LDS; dequantisation and the column pass (a thread per block column); the row pass, + 128 and the clamp of T.81 A.3.1 into three
// sample planes (a thread per block row); per pixel the chroma sample of its group, the colour transform, rounding, the clamp and
// three byte stores inside H x W.
template <int HS, int VS, bool GRAY>
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_pixels_kernel(JpegPixelParams p) {
  constexpr int MW = 8 * HS, MH = 8 * VS, NY = HS * VS, BPM = GRAY ? 1 : NY + 2, MPS = JPEG_DEC_STRIP_PX / MW, NB = MPS * BPM;
  __shared__ uint32_t s_coef[NB * 32];                           // int16 [NB][64]
  __shared__ float s_blk[NB * 64];                               // after the column pass: [block][y][u]
  __shared__ float s_plane[(MH + 16) * JPEG_DEC_PSTRIDE];        // rows [0, MH): Y; [MH, MH + 8): Cb; [MH + 8, MH + 16): Cr
  __shared__ float s_q[3][64];

  const int tid = threadIdx.x;
  const int64_t wg = blockIdx.x;
  const int strip = (int)(wg % p.strips), mrow = (int)((wg / p.strips) % p.mcu_rows);
  const int64_t n = wg / ((int64_t)p.strips * p.mcu_rows);
  const int left = p.mcu_cols - strip * MPS, nm = left < MPS ? left : MPS;   // MCUs of this strip inside the frame, >= 1
  if (tid < (GRAY ? 64 : 192)) s_q[tid >> 6][tid & 63] = (float)p.qtab[tid];
  const uint32_t* src = (const uint32_t*)(p.coef + ((n * p.mcu_rows + mrow) * p.mcu_cols + (int64_t)strip * MPS) * (BPM * 64));
  for (int i = tid; i < nm * BPM * 32; i += JPEG_THREADS) s_coef[i] = src[i];
  __syncthreads();

  const int16_t* coef = (const int16_t*)s_coef;
  for (int t = tid; t < nm * BPM * 8; t += JPEG_THREADS) {       // column pass: sum over v for every y, at column u
    const int b = t >> 3, u = t & 7, k = b % BPM;
    const float* q = s_q[k < NY ? 0 : k - NY + 1];
    float in[8], out[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int z = JPEG_ZIGZAG_POS[v * 8 + u];
      in[v] = (float)coef[b * 64 + z] * q[z];
    }
    jpeg_idct8(in, out);
#pragma unroll
    for (int y = 0; y < 8; ++y) s_blk[b * 64 + y * 8 + u] = out[y];
  }
  __syncthreads();

  for (int t = tid; t < nm * BPM * 8; t += JPEG_THREADS) {       // row pass: sum over u for every x, at row y
    const int b = t >> 3, y = t & 7, m = b / BPM, k = b - m * BPM;
    int row0, col0;
    if (k < NY) row0 = (k / HS) * 8, col0 = m * MW + (k % HS) * 8;
    else row0 = MH + 8 * (k - NY), col0 = m * 8;
    float in[8], out[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) in[u] = s_blk[b * 64 + y * 8 + u];
    jpeg_idct8(in, out);
    float* row = s_plane + (row0 + y) * JPEG_DEC_PSTRIDE + col0;
#pragma unroll
    for (int x = 0; x < 8; ++x) row[x] = fminf(fmaxf(out[x] + 128.0f, 0.0f), 255.0f);
  }
  __syncthreads();

  const int x0 = strip * JPEG_DEC_STRIP_PX, y0 = mrow * MH;
  const int wide = nm * MW;
  uint8_t* frame = p.out + n * p.frame_stride;
  for (int i = tid; i < MH * wide; i += JPEG_THREADS) {
    const int y = i / wide, x = i - y * wide;
    if (y0 + y >= p.H || x0 + x >= p.W) continue;
    const float Y = s_plane[y * JPEG_DEC_PSTRIDE + x];
    float R = Y, G = Y, B = Y;
    if (!GRAY) {
      const float cb = s_plane[(MH + y / VS) * JPEG_DEC_PSTRIDE + x / HS] - 128.0f;
      const float cr = s_plane[(MH + 8 + y / VS) * JPEG_DEC_PSTRIDE + x / HS] - 128.0f;
      R = fmaf(1.402f, cr, Y);
      G = fmaf(-0.714136286f, cr, fmaf(-0.344136286f, cb, Y));
      B = fmaf(1.772f, cb, Y);
    }
    uint8_t* px = frame + (int64_t)(y0 + y) * p.row_stride + (int64_t)(x0 + x) * 3;
    px[0] = (uint8_t)(int)fminf(fmaxf(rintf(R), 0.0f), 255.0f);
    px[1] = (uint8_t)(int)fminf(fmaxf(rintf(G), 0.0f), 255.0f);
    px[2] = (uint8_t)(int)fminf(fmaxf(rintf(B), 0.0f), 255.0f);
  }
}
