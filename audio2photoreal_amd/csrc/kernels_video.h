// Baseline JPEG on the GPU (include/a2p_hip.h "video frames"; host wrappers in a2p_video.h; audio2photoreal_amd/video.py):
// jpeg_coef_kernel      uint8 RGB frames -> quantised DCT coefficients in scan order (colour transform, chroma subsampling, 8 x 8 DCT,
//                       quantisation), fp32 with a fixed fmaf order;
// jpeg_entropy_kernel   those coefficients -> the Huffman-coded, byte-stuffed entropy segment of every frame, one restart interval per
//                       MCU row, one wave per interval; run once to size the intervals and once to write them;
// jpeg_offsets_kernel   the prefix sums between the two runs.
// Plain HIP C++: integer LDS atomics (an OR, independent of the order) and no float atomics; every frame's bytes are a function of
// that frame alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define JPEG_THREADS 256
#define JPEG_STRIP_PX 256          // pixels of an MCU row one workgroup of jpeg_coef_kernel owns
#define JPEG_STRIP_BLOCKS 96       // 8 x 8 blocks in a strip: 16 MCUs x 6 (4:2:0) or 32 MCUs x 3 (4:4:4)
#define JPEG_PSTRIDE 260           // floats between rows of the LDS planes: 256 + 4, so that the 8 rows of a block start 4 banks apart
#define JPEG_WAVE 64
// Capacity of one block's code, in bits.  The entropy kernel clamps a DC difference to +-2047 (category <= 11) and an AC coefficient
// to +-1023 (category <= 10) and cuts a Huffman code at 16 bits, so a block emits at most (16 + 11) + 63 (16 + 10) = 1665 bits: the DC
// symbol, then 63 non-zero AC coefficients (no ZRL fits between them and a non-zero coefficient 63 takes no EOB; a ZRL or the EOB
// replaces at least one 17-bit symbol by 16 bits).  The standard tables stay below it: 1660 (tests: the worst-case block).
#define JPEG_BLOCK_BITS 1665
#define JPEG_BIT_WORDS ((JPEG_WAVE * JPEG_BLOCK_BITS + 7 + 31) / 32 + 1)   // a chunk of 64 blocks, 7 carried bits, one spare word
#define JPEG_HUFF_WORDS 544        // DC luma [16], DC chroma [16], AC luma [256], AC chroma [256]: length << 16 | code

struct JpegCoefParams {
  const uint8_t* rgb;
  const uint16_t* qtab;            // [2][64], luma then chroma, natural (row-major v, u) order
  int16_t* out;
  int64_t frame_stride, row_stride;   // bytes
  int H, W, mcu_rows, mcu_cols, strips, aligned;
};

// scan position of the coefficient at natural index v * 8 + u
__device__ const uint8_t JPEG_ZIGZAG_POS[64] = {
    0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// out[u] = sum over x ascending of in[x] c[u][x], c[u][x] = C(u) / 2 cos((2 x + 1) u pi / 16): one fmaf per term after the first product
__device__ __forceinline__ void jpeg_dct8(const float (&in)[8], float (&out)[8]) {
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
  for (int u = 0; u < 8; ++u) {
    float a = in[0] * c[u][0];
#pragma unroll
    for (int x = 1; x < 8; ++x) a = fmaf(in[x], c[u][x], a);
    out[u] = a;
  }
}

// One workgroup per strip of 256 pixels of one MCU row.  SS = 2: 4:2:0 (MCU 16 x 16, blocks Y00 Y01 Y10 Y11 Cb Cr); SS = 1: 4:4:4
// (MCU 8 x 8, blocks Y Cb Cr).  Phases, each closed by a barrier: the strip's bytes to LDS (4-byte loads where the row allows them);
// colour transform and chroma mean to three float planes; the row pass of the DCT in place (a thread per block row); the column
// pass, quantisation and zig-zag to int16 in LDS (a thread per block column); 128-byte rows of coefficients to memory.
template <int SS>
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_coef_kernel(JpegCoefParams p) {
  constexpr int MH = 8 * SS, BPM = SS * SS + 2, MPS = JPEG_STRIP_PX / MH, ROW_BYTES = JPEG_STRIP_PX * 3, ROW_WORDS = ROW_BYTES / 4;
  static_assert(MPS * BPM == JPEG_STRIP_BLOCKS, "blocks of a strip");
  __shared__ uint32_t s_raw[16 * ROW_WORDS];                     // the strip's bytes; later the int16 coefficients [96][64]
  __shared__ __align__(16) float s_plane[(16 + 16) * JPEG_PSTRIDE];          // rows [0, MH): Y; [MH, MH + 8): Cb; [MH + 8, MH + 16): Cr
  __shared__ float s_q[2][64];
  static_assert(sizeof(s_raw) == JPEG_STRIP_BLOCKS * 64 * sizeof(int16_t), "the coefficient staging reuses the byte staging");

  const int tid = threadIdx.x;
  const int64_t wg = blockIdx.x;
  const int strip = (int)(wg % p.strips), mrow = (int)((wg / p.strips) % p.mcu_rows);
  const int64_t n = wg / ((int64_t)p.strips * p.mcu_rows);
  const int x0 = strip * JPEG_STRIP_PX, y0 = mrow * MH;
  const int rem = (p.W - x0) * 3 < ROW_BYTES ? (p.W - x0) * 3 : ROW_BYTES;     // bytes of the strip inside the image row, >= 3
  if (tid < 128) s_q[tid >> 6][tid & 63] = (float)p.qtab[tid];

  const uint8_t* frame = p.rgb + n * p.frame_stride + (int64_t)x0 * 3;
  for (int i = tid; i < MH * ROW_WORDS; i += JPEG_THREADS) {
    const int r = i / ROW_WORDS, d = i - r * ROW_WORDS;
    const int y = y0 + r < p.H ? y0 + r : p.H - 1;              // rows below the image repeat its last row
    const uint8_t* src = frame + (int64_t)y * p.row_stride + 4 * d;
    uint32_t w = 0;
    if (4 * d + 4 <= rem && p.aligned) {
      w = *(const uint32_t*)src;
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (4 * d + b < rem) w |= (uint32_t)src[b] << (8 * b);
    }
    s_raw[i] = w;
  }
  __syncthreads();

  {
    const uint8_t* raw = (const uint8_t*)s_raw;
    constexpr int GW = JPEG_STRIP_PX / SS;                       // chroma samples per row; 8 chroma rows
    const int xmax = p.W - 1 - x0;                               // columns right of the image repeat its last column
    for (int g = tid; g < 8 * GW; g += JPEG_THREADS) {
      const int gy = g / GW, gx = g - gy * GW;
      float cb[SS * SS], cr[SS * SS];
#pragma unroll
      for (int dy = 0; dy < SS; ++dy)
#pragma unroll
        for (int dx = 0; dx < SS; ++dx) {
          const int yy = gy * SS + dy, xx = gx * SS + dx, xc = xx < xmax ? xx : xmax;
          const uint8_t* px = raw + yy * ROW_BYTES + 3 * xc;
          const float R = (float)px[0], G = (float)px[1], B = (float)px[2];
          const float Y = fmaf(0.114f, B, fmaf(0.587f, G, 0.299f * R));
          cb[dy * SS + dx] = fmaf(0.5f, B, fmaf(-0.331264108f, G, -0.168735892f * R)) + 128.0f;
          cr[dy * SS + dx] = fmaf(-0.081312411f, B, fmaf(-0.418687589f, G, 0.5f * R)) + 128.0f;
          s_plane[yy * JPEG_PSTRIDE + xx] = Y - 128.0f;
        }
      float mb, mr;
      if (SS == 2) {
        mb = ((cb[0] + cb[1]) + (cb[2] + cb[3])) * 0.25f;
        mr = ((cr[0] + cr[1]) + (cr[2] + cr[3])) * 0.25f;
      } else {
        mb = cb[0], mr = cr[0];
      }
      s_plane[(MH + gy) * JPEG_PSTRIDE + gx] = mb - 128.0f;
      s_plane[(MH + 8 + gy) * JPEG_PSTRIDE + gx] = mr - 128.0f;
    }
  }
  __syncthreads();

  const int left = p.mcu_cols - strip * MPS, nm = left < MPS ? left : MPS;   // MCUs of this strip inside the frame
  // block b of the strip: MCU m = b / BPM, k = b % BPM; its top-left sample in s_plane
  auto origin = [&](int b, int& row0, int& col0, int& table) {
    const int m = b / BPM, k = b - m * BPM;
    if (k < SS * SS) row0 = (k / SS) * 8, col0 = m * MH + (k % SS) * 8, table = 0;
    else row0 = MH + 8 * (k - SS * SS), col0 = m * 8, table = 1;
  };
  for (int t = tid; t < nm * BPM * 8; t += JPEG_THREADS) {       // row pass, in place: the thread owns the 8 samples it reads
    int row0, col0, table;
    origin(t >> 3, row0, col0, table);
    float* row = s_plane + (row0 + (t & 7)) * JPEG_PSTRIDE + col0;
    float in[8], out[8];
    *(float4*)&in[0] = *(const float4*)row, *(float4*)&in[4] = *(const float4*)(row + 4);
    jpeg_dct8(in, out);
    *(float4*)row = *(const float4*)&out[0], *(float4*)(row + 4) = *(const float4*)&out[4];
  }
  __syncthreads();

  int16_t* s_coef = (int16_t*)s_raw;
  for (int t = tid; t < nm * BPM * 8; t += JPEG_THREADS) {       // column pass
    int row0, col0, table;
    const int b = t >> 3, u = t & 7;
    origin(b, row0, col0, table);
    const float* col = s_plane + row0 * JPEG_PSTRIDE + col0 + u;
    float in[8], out[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) in[y] = col[y * JPEG_PSTRIDE];
    jpeg_dct8(in, out);
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      float q = rintf(out[v] / s_q[table][v * 8 + u]);
      if (v + u) q = fminf(fmaxf(q, -1023.0f), 1023.0f);
      s_coef[b * 64 + JPEG_ZIGZAG_POS[v * 8 + u]] = (int16_t)(int)q;
    }
  }
  __syncthreads();

  uint32_t* dst = (uint32_t*)(p.out + ((n * p.mcu_rows + mrow) * p.mcu_cols + (int64_t)strip * MPS) * (BPM * 64));
  for (int i = tid; i < nm * BPM * 32; i += JPEG_THREADS) dst[i] = s_raw[i];
}

// ------------------------------------------------------------------------------------------------ entropy coding
struct JpegEntropyParams {
  const int16_t* coef;             // [N, mcu_rows, mcu_cols, bpm, 64]
  const uint32_t* huff;            // [JPEG_HUFF_WORDS]
  const uint8_t* head;             // head_bytes copied in front of every frame's segment, tail_bytes behind it (NULL: left untouched)
  const uint8_t* tail;
  int64_t* interval;               // [N, mcu_rows]: sizing writes the intervals' byte lengths, jpeg_offsets_kernel turns them into offsets
  int64_t* offsets;                // [N + 1]: where every frame (head included) starts in out
  uint8_t* out;
  int64_t out_bytes;
  int64_t N;
  int mcu_rows, mcu_cols, bpm, head_bytes, tail_bytes;
};

__device__ __forceinline__ int jpeg_wave_scan(int v, int lane) {   // inclusive prefix sum over the wave
#pragma unroll
  for (int d = 1; d < JPEG_WAVE; d <<= 1) {
    const int t = __shfl_up(v, d, JPEG_WAVE);
    if (lane >= d) v += t;
  }
  return v;
}

struct JpegCountBits {
  int bits = 0;
  __device__ __forceinline__ void operator()(uint32_t, int len) { bits += len; }
};

// Appends codes of 1..27 bits at bit position `pos` of a zeroed big-endian word array.  Full words are OR-ed into LDS once; only the
// first and last word of a lane's string are shared with its neighbours, and an OR does not depend on the order.
struct JpegPutBits {
  uint32_t* buf;
  uint32_t pos, acc = 0;
  __device__ __forceinline__ JpegPutBits(uint32_t* b, uint32_t start) : buf(b), pos(start) {}
  __device__ __forceinline__ void operator()(uint32_t bits, int len) {
    if (len == 0) return;
    const uint32_t w = pos >> 5;
    const uint64_t v = (uint64_t)bits << (64 - len - (int)(pos & 31));    // len + (pos & 31) <= 58
    acc |= (uint32_t)(v >> 32);
    pos += (uint32_t)len;
    if ((pos >> 5) != w) {
      atomicOr(&buf[w], acc);
      acc = (uint32_t)v;
    }
  }
  __device__ __forceinline__ void flush() {
    if (acc) atomicOr(&buf[pos >> 5], acc);
  }
};

// The symbols of one block: the DC difference (category, amplitude), then (run, size) symbols with ZRL for runs of 16 and EOB for a
// zero tail.  row: the block's 64 coefficients in scan order.
template <class Put>
__device__ __forceinline__ void jpeg_code_block(const int16_t* row, int diff, const uint32_t* hdc, const uint32_t* hac, Put& put) {
  auto sym = [&](uint32_t h, uint32_t amp, int s) {
    int len = (int)(h >> 16) & 31;
    len = len < 16 ? len : 16;
    put((((h & 0xffffu) & ((1u << len) - 1u)) << s) | amp, len + s);
  };
  diff = diff < -2047 ? -2047 : (diff > 2047 ? 2047 : diff);
  {
    const int a = diff < 0 ? -diff : diff, s = 32 - __clz(a);
    sym(hdc[s], (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u), s);
  }
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    int v = row[k];
    if (v == 0) {
      ++run;
      continue;
    }
    for (; run >= 16; run -= 16) sym(hac[0xF0], 0, 0);
    v = v < -1023 ? -1023 : (v > 1023 ? 1023 : v);
    const int a = v < 0 ? -v : v, s = 32 - __clz(a);
    sym(hac[(run << 4) | s], (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u), s);
    run = 0;
  }
  if (run) sym(hac[0], 0, 0);
}

// One wave per restart interval (one MCU row of one frame), a lane per block, 64 blocks at a time: the lanes measure their blocks'
// codes, a wave prefix sum places them, the lanes OR them into the chunk's bit buffer in LDS; a second prefix sum over the 0xFF
// bytes of 64 byte ranges drives the stuffing.  The bits of a chunk that do not fill a byte are carried into the next one; the last
// chunk is padded with 1-bits, and every interval but the frame's last is followed by RSTm, m = row mod 8.
// WRITE = false: only the interval's byte length is computed (interval[]); WRITE = true: the bytes are written at offsets[n] +
// head_bytes + interval[] (then an offset), and the first / last interval of a frame copies the head / tail.  No byte at or beyond
// out_bytes is written.
template <bool WRITE>
__global__ __launch_bounds__(JPEG_WAVE) void jpeg_entropy_kernel(JpegEntropyParams p) {
  __shared__ uint32_t s_huff[JPEG_HUFF_WORDS];
  __shared__ uint32_t s_bits[JPEG_BIT_WORDS];
  __shared__ uint32_t s_coef[JPEG_WAVE * 33];                    // 64 rows of 32 words, one word of padding: a lane per row, no conflicts
  const int lane = threadIdx.x;
  const int64_t iv = blockIdx.x, n = iv / p.mcu_rows;
  const int r = (int)(iv - n * p.mcu_rows), nblk = p.mcu_cols * p.bpm, ny = p.bpm - 2;
  for (int i = lane; i < JPEG_HUFF_WORDS; i += JPEG_WAVE) s_huff[i] = p.huff[i];
  const int16_t* src = p.coef + iv * nblk * 64;

  int64_t pos = 0;                                               // bytes of this interval so far
  int64_t base = 0;
  if (WRITE) {
    base = p.offsets[n] + p.head_bytes + p.interval[iv];
    if (r == 0 && p.head)
      for (int i = lane; i < p.head_bytes; i += JPEG_WAVE)
        if (p.offsets[n] + i >= 0 && p.offsets[n] + i < p.out_bytes) p.out[p.offsets[n] + i] = p.head[i];
    if (r == p.mcu_rows - 1 && p.tail)
      for (int i = lane; i < p.tail_bytes; i += JPEG_WAVE) {
        const int64_t at = p.offsets[n + 1] - p.tail_bytes + i;
        if (at >= 0 && at < p.out_bytes) p.out[at] = p.tail[i];
      }
  }
  auto store = [&](int64_t at, uint32_t byte) {
    if (base + at >= 0 && base + at < p.out_bytes) p.out[base + at] = (uint8_t)byte;
  };
  auto byte_at = [&](int i) { return (s_bits[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu; };

  int carry_bits = 0;
  uint32_t carry = 0;                                            // the carried bits, at the top of a byte
  for (int c0 = 0; c0 < nblk; c0 += JPEG_WAVE) {
    const int nb = nblk - c0 < JPEG_WAVE ? nblk - c0 : JPEG_WAVE;
    const bool last = c0 + JPEG_WAVE >= nblk;
    __syncthreads();                                             // the previous chunk's bytes are read; s_huff is loaded
    for (int i = lane; i < nb * 32; i += JPEG_WAVE) s_coef[(i >> 5) * 33 + (i & 31)] = ((const uint32_t*)src)[(int64_t)c0 * 32 + i];
    __syncthreads();

    const int16_t* row = (const int16_t*)(s_coef + lane * 33);
    const int k = (c0 + lane) % p.bpm, luma = k < ny;
    const uint32_t* hdc = s_huff + (luma ? 0 : 16);
    const uint32_t* hac = s_huff + 32 + (luma ? 0 : 256);
    int diff = 0, bits = 0;
    if (lane < nb) {
      // the block of the same component before this one: the previous block inside an MCU's luma, else the same place one MCU back
      const int prev = c0 + lane - (luma ? (k > 0 ? 1 : 3) : p.bpm);
      diff = row[0] - (prev >= 0 ? (int)src[(int64_t)prev * 64] : 0);
      JpegCountBits count;
      jpeg_code_block(row, diff, hdc, hac, count);
      bits = count.bits;
    }
    const int incl = jpeg_wave_scan(bits, lane);
    const int total = carry_bits + __shfl(incl, JPEG_WAVE - 1, JPEG_WAVE);
    for (int i = lane; i <= (total >> 5) + 1; i += JPEG_WAVE) s_bits[i] = i == 0 ? carry << 24 : 0u;
    __syncthreads();
    if (lane < nb) {
      JpegPutBits put(s_bits, (uint32_t)(carry_bits + incl - bits));
      jpeg_code_block(row, diff, hdc, hac, put);
      put.flush();
    }
    __syncthreads();

    int nbytes = total >> 3;
    const int rest = total & 7;
    if (last && rest) {                                          // pad the interval with 1-bits
      if (lane == 0) s_bits[nbytes >> 2] |= ((1u << (8 - rest)) - 1u) << (24 - 8 * (nbytes & 3));
      ++nbytes;
      __syncthreads();
    }
    const int per = (nbytes + JPEG_WAVE - 1) / JPEG_WAVE;
    const int b0 = lane * per < nbytes ? lane * per : nbytes, b1 = b0 + per < nbytes ? b0 + per : nbytes;
    int ff = 0;
    for (int i = b0; i < b1; ++i) ff += byte_at(i) == 0xffu;
    const int ffi = jpeg_wave_scan(ff, lane);
    if (WRITE) {
      int64_t at = pos + b0 + (ffi - ff);
      for (int i = b0; i < b1; ++i) {
        const uint32_t b = byte_at(i);
        store(at++, b);
        if (b == 0xffu) store(at++, 0u);                         // byte stuffing
      }
    }
    pos += nbytes + __shfl(ffi, JPEG_WAVE - 1, JPEG_WAVE);
    carry_bits = last ? 0 : rest;
    carry = carry_bits ? byte_at(nbytes) & (0xff00u >> carry_bits) & 0xffu : 0u;
  }
  if (r != p.mcu_rows - 1) {
    if (WRITE && lane == 0) store(pos, 0xffu), store(pos + 1, 0xd0u + (uint32_t)(r & 7));
    pos += 2;
  }
  if (!WRITE && lane == 0) p.interval[iv] = pos;
}

// One workgroup: interval[n][r] lengths -> offsets inside the frame's segment; offsets[n] = sum over m < n of (head + segment + tail).
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_offsets_kernel(JpegEntropyParams p) {
  __shared__ int64_t s_sum[JPEG_THREADS];
  const int tid = threadIdx.x;
  for (int64_t n = tid; n < p.N; n += JPEG_THREADS) {
    int64_t run = 0;
    for (int r = 0; r < p.mcu_rows; ++r) {
      const int64_t len = p.interval[n * p.mcu_rows + r];
      p.interval[n * p.mcu_rows + r] = run;
      run += len;
    }
    p.offsets[n + 1] = run + p.head_bytes + p.tail_bytes;
  }
  __syncthreads();
  int64_t carry = 0;
  for (int64_t n0 = 0; n0 < p.N; n0 += JPEG_THREADS) {
    const bool in = n0 + tid < p.N;
    s_sum[tid] = in ? p.offsets[n0 + tid + 1] : 0;
    __syncthreads();
    for (int d = 1; d < JPEG_THREADS; d <<= 1) {
      const int64_t t = tid >= d ? s_sum[tid - d] : 0;
      __syncthreads();
      s_sum[tid] += t;
      __syncthreads();
    }
    if (in) p.offsets[n0 + tid + 1] = carry + s_sum[tid];
    carry += s_sum[JPEG_THREADS - 1];
    __syncthreads();
  }
  if (tid == 0) p.offsets[0] = 0;
}
