// The integer half of the baseline JPEG decoder (include/a2p_hip.h "reading video frames"), as plain C++ that the kernels of
// kernels_video_decode.h and a host program (tests/tools/jpeg_decode_host.cpp, built with sanitizers) both compile: the restart
// scan, the bit reader, the Huffman lookup and the block loop.  Pointers and lengths only, no HIP intrinsics, no allocation.
// Nothing here trusts its input: every byte index is compared with the interval's end before the byte is read, every loop is
// bounded by the geometry (at most 64 symbols a block, every symbol at least one bit), and a table index is masked to the table.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ __forceinline__
#else
#define JPEG_HD inline
#endif

// cause codes of a frame's status: status = (interval << 4) | cause, 0 = decoded
#define JPEG_OK 0
#define JPEG_ERR_RST_COUNT 1       // fewer or more RSTm markers than ceil(mcus / Ri) - 1
#define JPEG_ERR_RST_ORDER 2       // RSTm out of the cyclic order RST0 .. RST7
#define JPEG_ERR_MARKER 3          // 0xFF followed by anything but 0x00 or the RSTm due (another marker, a fill byte, the segment's end)
#define JPEG_ERR_NO_CODE 4         // 16 bits that start no code of the table
#define JPEG_ERR_RUN 5             // a run that takes the coefficient index past 63
#define JPEG_ERR_ENDS_IN_CODE 6    // the interval ends inside a code or an amplitude
#define JPEG_ERR_AMPLITUDE 7       // a DC category above 11, an AC size above 10 or a DC value outside int16: not 8-bit baseline
#define JPEG_ERR_TRAILING 8        // a whole byte or more left behind the interval's last block
#define JPEG_STATUS(interval, cause) ((int32_t)(((int64_t)(interval) << 4) | (cause)))

// A Huffman table as the decoder holds it, JPEG_TABLE_WORDS int32: maxcode[16] (the largest code of length l + 1, -1 for none),
// offset[16] (index into vals of that length's first symbol minus its first code), vals[256] as bytes.  Four of them: DC 0, DC 1,
// AC 0, AC 1 (Tc * 2 + Th).
#define JPEG_TABLE_WORDS 96
#define JPEG_TABLES 4

// what one byte of an entropy-coded segment starts: decided from the byte and its successor alone, so a scan can run in parallel
#define JPEG_BYTE_DATA (-1)
#define JPEG_BYTE_BAD (-2)
JPEG_HD int jpeg_classify(const uint8_t* data, int64_t i, int64_t end) {      // i < end; returns m of RSTm, or JPEG_BYTE_*
  if (data[i] != 0xFF) return JPEG_BYTE_DATA;
  if (i + 1 >= end) return JPEG_BYTE_BAD;
  const int next = data[i + 1];
  if (next == 0x00) return JPEG_BYTE_DATA;
  return next >= 0xD0 && next <= 0xD7 ? next - 0xD0 : JPEG_BYTE_BAD;
}

// The verdict on one byte given how many RSTm precede it: 0, or the status it contributes.  The frame's status is the smallest
// non-zero one, then the count's.
JPEG_HD int32_t jpeg_restart_verdict(int kind, int64_t before, int64_t intervals) {
  if (kind == JPEG_BYTE_DATA) return 0;
  const int64_t iv = before < intervals - 1 ? before : intervals - 1;
  if (kind == JPEG_BYTE_BAD) return JPEG_STATUS(iv, JPEG_ERR_MARKER);
  if (before >= intervals - 1) return JPEG_STATUS(iv, JPEG_ERR_RST_COUNT);
  return kind == (int)(before & 7) ? 0 : JPEG_STATUS(iv, JPEG_ERR_RST_ORDER);
}

// Sequential restart scan of data[begin, end): ranges[k], k < intervals, is where interval k starts (ranges[0] = begin, then the
// byte behind the k-th marker) and ranges[intervals] = end; interval k ends 2 bytes (its marker) before ranges[k + 1], the last one
// at end.  Returns the status; ranges are complete only when it is 0.
JPEG_HD int32_t jpeg_restart_ranges(const uint8_t* data, int64_t begin, int64_t end, int64_t intervals, int64_t* ranges) {
  int64_t count = 0;
  int32_t worst = 0;
  ranges[0] = begin, ranges[intervals] = end;
  for (int64_t i = begin; i < end; ++i) {
    const int kind = jpeg_classify(data, i, end);
    const int32_t v = jpeg_restart_verdict(kind, count, intervals);
    if (v && (!worst || v < worst)) worst = v;
    if (kind >= 0) {
      if (count + 1 < intervals) ranges[count + 1] = i + 2;
      ++count;
    }
  }
  if (worst) return worst;
  return count == intervals - 1 ? 0 : JPEG_STATUS(count < intervals - 1 ? count : intervals - 1, JPEG_ERR_RST_COUNT);
}

// ------------------------------------------------------------------------------------------------ bits
struct JpegBits {
  const uint8_t* data;
  int64_t pos, end;                // the next byte and the interval's end
  uint64_t acc;                    // the low n bits are the bits not yet consumed
  int n;
};

JPEG_HD void jpeg_bits_open(JpegBits& b, const uint8_t* data, int64_t begin, int64_t end) {
  b.data = data, b.pos = begin, b.end = end > begin ? end : begin, b.acc = 0, b.n = 0;
}

// Takes bytes until 49 or more bits are held or the interval ends; 0xFF 0x00 is one data byte, 0xFF before anything else ends the data.
JPEG_HD void jpeg_bits_fill(JpegBits& b) {
  while (b.n <= 48 && b.pos < b.end) {
    const uint32_t c = b.data[b.pos];
    if (c == 0xFF) {
      if (b.pos + 1 < b.end && b.data[b.pos + 1] == 0x00) {
        b.pos += 2;
      } else {
        b.end = b.pos;
        break;
      }
    } else {
      b.pos += 1;
    }
    b.acc = (b.acc << 8) | c;
    b.n += 8;
  }
}

// k <= 16 bits, or -1 where the interval holds fewer
JPEG_HD int jpeg_bits_take(JpegBits& b, int k) {
  if (k == 0) return 0;
  if (b.n < k) jpeg_bits_fill(b);
  if (b.n < k) return -1;
  b.n -= k;
  return (int)((b.acc >> b.n) & ((1u << k) - 1u));
}

// One symbol of `table`, or -cause
JPEG_HD int jpeg_huff_symbol(JpegBits& b, const int32_t* table) {
  if (b.n < 16) jpeg_bits_fill(b);
  const uint32_t peek = b.n >= 16 ? (uint32_t)(b.acc >> (b.n - 16)) & 0xffffu
                                  : (((uint32_t)b.acc << (16 - b.n)) | ((1u << (16 - b.n)) - 1u)) & 0xffffu;
  const uint8_t* vals = (const uint8_t*)(table + 32);
  for (int l = 1; l <= 16; ++l) {
    const int32_t code = (int32_t)(peek >> (16 - l)), top = table[l - 1];
    if (top >= 0 && code <= top) {
      if (l > b.n) return -JPEG_ERR_ENDS_IN_CODE;
      b.n -= l;
      return vals[(uint32_t)(code + table[16 + l - 1]) & 255u];
    }
  }
  return b.n >= 16 ? -JPEG_ERR_NO_CODE : -JPEG_ERR_ENDS_IN_CODE;
}

JPEG_HD int jpeg_extend(int bits, int size) {                               // F.2.2.1
  return size == 0 || (bits >> (size - 1)) ? bits : bits - (1 << size) + 1;
}

// One block: the DC difference on top of `pred`, then (run, size) symbols up to EOB or coefficient 63.  out: the block's 64
// coefficients in scan order, zero before the call; only non-zero values are stored.  Returns the cause, 0 when the block decoded.
JPEG_HD int jpeg_decode_block(JpegBits& b, const int32_t* dc, const int32_t* ac, int& pred, int16_t* out) {
  int size = jpeg_huff_symbol(b, dc);
  if (size < 0) return -size;
  if (size > 11) return JPEG_ERR_AMPLITUDE;
  int bits = jpeg_bits_take(b, size);
  if (bits < 0) return JPEG_ERR_ENDS_IN_CODE;
  pred += jpeg_extend(bits, size);
  if (pred < -32768 || pred > 32767) return JPEG_ERR_AMPLITUDE;
  if (pred) out[0] = (int16_t)pred;
  int j = 1;
  for (int symbols = 0; symbols < 63 && j < 64; ++symbols) {                 // every symbol moves j by at least 1
    const int rs = jpeg_huff_symbol(b, ac);
    if (rs < 0) return -rs;
    const int run = rs >> 4;
    size = rs & 15;
    if (size == 0) {
      if (run != 15) break;                                                  // EOB
      j += 16;                                                               // ZRL
      continue;
    }
    if (size > 10) return JPEG_ERR_AMPLITUDE;
    j += run;
    if (j > 63) return JPEG_ERR_RUN;
    bits = jpeg_bits_take(b, size);
    if (bits < 0) return JPEG_ERR_ENDS_IN_CODE;
    const int v = jpeg_extend(bits, size);                                   // never 0: size >= 1
    out[j++] = (int16_t)v;
  }
  return 0;
}

struct JpegScan {
  int bpm, ny;                     // blocks of an MCU; the first ny are component 0, then one block each of components 1 and 2
  int dc[3], ac[3];                // the table (0 or 1) of every component
};

// One restart interval: MCUs [m0, m1) of a frame whose coefficients [mcus, bpm, 64] start at `coef` (zero before the call), read
// from data[begin, end).  The DC prediction of every component starts at 0.  Returns the cause.
JPEG_HD int jpeg_decode_interval(const uint8_t* data, int64_t begin, int64_t end, const int32_t* tables, const JpegScan& sc, int64_t m0,
                                 int64_t m1, int16_t* coef) {
  JpegBits b;
  jpeg_bits_open(b, data, begin, end);
  int pred[3] = {0, 0, 0};
  for (int64_t m = m0; m < m1; ++m)
    for (int k = 0; k < sc.bpm; ++k) {
      const int c = k < sc.ny ? 0 : k - sc.ny + 1;
      const int cause = jpeg_decode_block(b, tables + (sc.dc[c] & 1) * JPEG_TABLE_WORDS, tables + (2 + (sc.ac[c] & 1)) * JPEG_TABLE_WORDS,
                                          pred[c], coef + (m * sc.bpm + k) * 64);
      if (cause) return cause;
    }
  jpeg_bits_fill(b);
  return b.n >= 8 || b.pos < b.end ? JPEG_ERR_TRAILING : 0;
}
