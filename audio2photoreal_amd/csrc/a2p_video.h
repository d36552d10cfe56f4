// C ABI of the video frames (include/a2p_hip.h "video frames" and "reading video frames"; kernels in kernels_video.h and
// kernels_video_decode.h).  Context-free like the encode layers:
// the quantisation and Huffman tables are device arrays the caller prepared once (audio2photoreal_amd/video.py builds them on the
// host).  Included at the end of a2p_lib.hip after a2p_encode.h (set_err / ARG / HIPCHK).
#pragma once

static inline bool jpeg_bytes_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  if (!a || !b || na <= 0 || nb <= 0) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

extern "C" int a2p_jpeg_coefficients(const uint8_t* rgb, int64_t N, int32_t H, int32_t W, int64_t frame_stride, int64_t row_stride,
                                     int32_t subsampling, const uint16_t* qtab, int16_t* out, void* stream) {
  static_assert(JPEG_BLOCK_BITS == A2P_JPEG_BLOCK_BITS && JPEG_HUFF_WORDS == A2P_JPEG_HUFF_WORDS, "jpeg constants");
  ARG(rgb && qtab && out, "jpeg_coefficients: null rgb, qtab or out");
  ARG(N >= 0, "jpeg_coefficients: N=%lld is negative", (long long)N);
  ARG(H >= 1 && H <= A2P_JPEG_MAX_SIZE && W >= 1 && W <= A2P_JPEG_MAX_SIZE, "jpeg_coefficients: the frames are %d x %d, outside [1, %d]", H,
      W, A2P_JPEG_MAX_SIZE);
  ARG(subsampling == 420 || subsampling == 444, "jpeg_coefficients: subsampling=%d, need 420 or 444", subsampling);
  ARG(row_stride >= (int64_t)3 * W, "jpeg_coefficients: row_stride=%lld bytes is below 3 W = %d", (long long)row_stride, 3 * W);
  const int64_t frame = (int64_t)(H - 1) * row_stride + (int64_t)3 * W;
  ARG(frame_stride >= frame || N <= 1, "jpeg_coefficients: frame_stride=%lld bytes is below (H - 1) row_stride + 3 W = %lld",
      (long long)frame_stride, (long long)frame);
  ARG((uintptr_t)out % 4 == 0, "jpeg_coefficients: out must be 4-byte aligned");
  const int mcu = subsampling == 420 ? 16 : 8, bpm = subsampling == 420 ? 6 : 3;
  JpegCoefParams p = {};
  p.mcu_rows = (H + mcu - 1) / mcu, p.mcu_cols = (W + mcu - 1) / mcu;
  p.strips = (W + JPEG_STRIP_PX - 1) / JPEG_STRIP_PX;
  ARG(N * p.mcu_rows * p.strips <= 0x7fffffff, "jpeg_coefficients: N=%lld frames x %d MCU rows x %d strips exceed the grid", (long long)N,
      p.mcu_rows, p.strips);
  const int64_t out_bytes = N * p.mcu_rows * p.mcu_cols * bpm * 128, in_bytes = N > 0 ? (N - 1) * frame_stride + frame : 0;
  ARG(!jpeg_bytes_overlap(out, out_bytes, rgb, in_bytes), "jpeg_coefficients: out must not alias an input (it overlaps rgb)");
  ARG(!jpeg_bytes_overlap(out, out_bytes, qtab, 256), "jpeg_coefficients: out must not alias an input (it overlaps qtab)");
  if (N == 0) return 0;
  p.rgb = rgb, p.qtab = qtab, p.out = out, p.frame_stride = frame_stride, p.row_stride = row_stride, p.H = H, p.W = W;
  p.aligned = (uintptr_t)rgb % 4 == 0 && frame_stride % 4 == 0 && row_stride % 4 == 0;   // only the loads differ, never the arithmetic
  const unsigned grid = (unsigned)(N * p.mcu_rows * p.strips);
  if (subsampling == 420) jpeg_coef_kernel<2><<<grid, JPEG_THREADS, 0, (hipStream_t)stream>>>(p);
  else jpeg_coef_kernel<1><<<grid, JPEG_THREADS, 0, (hipStream_t)stream>>>(p);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_jpeg_entropy(const int16_t* coef, int64_t N, int32_t mcu_rows, int32_t mcu_cols, int32_t blocks_per_mcu,
                                const uint32_t* huff, const uint8_t* head, int32_t head_bytes, const uint8_t* tail, int32_t tail_bytes,
                                int64_t* interval, int64_t* offsets, uint8_t* out, int64_t out_bytes, void* stream) {
  ARG(coef && huff && interval && offsets, "jpeg_entropy: null coef, huff, interval or offsets");
  ARG(N >= 0, "jpeg_entropy: N=%lld is negative", (long long)N);
  ARG(mcu_rows >= 1 && mcu_rows <= A2P_JPEG_MAX_SIZE / 8 + 1 && mcu_cols >= 1 && mcu_cols <= A2P_JPEG_MAX_SIZE / 8 + 1,
      "jpeg_entropy: %d x %d MCUs, outside [1, %d]", mcu_rows, mcu_cols, A2P_JPEG_MAX_SIZE / 8 + 1);
  ARG(blocks_per_mcu == 3 || blocks_per_mcu == 6, "jpeg_entropy: blocks_per_mcu=%d, need 3 (4:4:4) or 6 (4:2:0)", blocks_per_mcu);
  ARG(head_bytes >= 0 && tail_bytes >= 0 && head_bytes <= 65536 && tail_bytes <= 65536, "jpeg_entropy: head_bytes=%d, tail_bytes=%d, outside [0, 65536]",
      head_bytes, tail_bytes);
  ARG(N * mcu_rows <= 0x7fffffff, "jpeg_entropy: N=%lld frames x %d MCU rows exceed the grid", (long long)N, mcu_rows);
  ARG((uintptr_t)coef % 4 == 0, "jpeg_entropy: coef must be 4-byte aligned");
  ARG(!out || out_bytes >= 0, "jpeg_entropy: out_bytes=%lld is negative", (long long)out_bytes);
  const int64_t coef_bytes = N * mcu_rows * mcu_cols * blocks_per_mcu * 128;
  const struct { const char* name; const void* ptr; int64_t n; } inputs[] = {
      {"coef", coef, coef_bytes}, {"huff", huff, JPEG_HUFF_WORDS * 4}, {"head", head, head_bytes}, {"tail", tail, tail_bytes}};
  for (const auto& in : inputs) {
    ARG(!jpeg_bytes_overlap(out, out_bytes, in.ptr, in.n), "jpeg_entropy: out must not alias an input (it overlaps %s)", in.name);
    ARG(!jpeg_bytes_overlap(interval, N * mcu_rows * 8, in.ptr, in.n), "jpeg_entropy: interval must not alias an input (it overlaps %s)", in.name);
    ARG(!jpeg_bytes_overlap(offsets, (N + 1) * 8, in.ptr, in.n), "jpeg_entropy: offsets must not alias an input (it overlaps %s)", in.name);
  }
  ARG(!jpeg_bytes_overlap(interval, N * mcu_rows * 8, offsets, (N + 1) * 8), "jpeg_entropy: interval must not alias offsets");
  ARG(!jpeg_bytes_overlap(out, out_bytes, offsets, (N + 1) * 8) && !jpeg_bytes_overlap(out, out_bytes, interval, N * mcu_rows * 8),
      "jpeg_entropy: out must not alias interval or offsets");
  JpegEntropyParams p = {};
  p.coef = coef, p.huff = huff, p.head = head, p.tail = tail, p.interval = interval, p.offsets = offsets, p.out = out, p.out_bytes = out_bytes;
  p.N = N, p.mcu_rows = mcu_rows, p.mcu_cols = mcu_cols, p.bpm = blocks_per_mcu, p.head_bytes = head_bytes, p.tail_bytes = tail_bytes;
  hipStream_t s = (hipStream_t)stream;
  if (!out) {                                                    // sizing
    if (N > 0) jpeg_entropy_kernel<false><<<(unsigned)(N * mcu_rows), JPEG_WAVE, 0, s>>>(p);
    jpeg_offsets_kernel<<<1, JPEG_THREADS, 0, s>>>(p);
  } else if (N > 0) {
    jpeg_entropy_kernel<true><<<(unsigned)(N * mcu_rows), JPEG_WAVE, 0, s>>>(p);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------------ reading (kernels_video_decode.h)
extern "C" int a2p_jpeg_restarts(const uint8_t* data, int64_t data_bytes, const int64_t* segments, int64_t N, int64_t intervals,
                                 int64_t* ranges, int32_t* status, void* stream) {
  ARG(data && segments && ranges && status, "jpeg_restarts: null data, segments, ranges or status");
  ARG(N >= 0 && N <= 0x7fffffff, "jpeg_restarts: N=%lld is outside [0, 2^31)", (long long)N);
  ARG(data_bytes >= 0, "jpeg_restarts: data_bytes=%lld is negative", (long long)data_bytes);
  ARG(intervals >= 1 && intervals <= ((int64_t)1 << 26), "jpeg_restarts: intervals=%lld is outside [1, 2^26]", (long long)intervals);
  const int64_t range_bytes = N * (intervals + 1) * 8;
  ARG(!jpeg_bytes_overlap(ranges, range_bytes, data, data_bytes) && !jpeg_bytes_overlap(ranges, range_bytes, segments, N * 16) &&
          !jpeg_bytes_overlap(status, N * 4, data, data_bytes) && !jpeg_bytes_overlap(status, N * 4, segments, N * 16) &&
          !jpeg_bytes_overlap(status, N * 4, ranges, range_bytes),
      "jpeg_restarts: ranges and status must not alias an input or each other");
  if (N == 0) return 0;
  JpegRestartParams p = {};
  p.data = data, p.data_bytes = data_bytes, p.segments = segments, p.intervals = intervals, p.ranges = ranges, p.status = status;
  jpeg_restarts_kernel<<<(unsigned)N, JPEG_THREADS, 0, (hipStream_t)stream>>>(p);
  HIPCHK(hipGetLastError());
  return 0;
}

// blocks of an MCU -> luminance blocks; 0 for a layout that is not read
static inline int jpeg_luma_blocks(int bpm) { return bpm == 1 ? 1 : (bpm == 3 || bpm == 4 || bpm == 6 ? bpm - 2 : 0); }

extern "C" int a2p_jpeg_decode_entropy(const uint8_t* data, int64_t data_bytes, const int64_t* ranges, const int32_t* restart_status,
                                       int64_t N, int32_t mcu_rows, int32_t mcu_cols, int32_t blocks_per_mcu, int32_t restart_interval,
                                       const int32_t* tables, int32_t selectors, int16_t* coef, int32_t* status, void* stream) {
  static_assert(JPEG_TABLE_WORDS == A2P_JPEG_TABLE_WORDS && JPEG_TABLES == A2P_JPEG_TABLES, "jpeg constants");
  ARG(data && ranges && tables && coef && status, "jpeg_decode_entropy: null data, ranges, tables, coef or status");
  ARG(N >= 0, "jpeg_decode_entropy: N=%lld is negative", (long long)N);
  ARG(data_bytes >= 0, "jpeg_decode_entropy: data_bytes=%lld is negative", (long long)data_bytes);
  ARG(mcu_rows >= 1 && mcu_rows <= A2P_JPEG_MAX_SIZE / 8 + 1 && mcu_cols >= 1 && mcu_cols <= A2P_JPEG_MAX_SIZE / 8 + 1,
      "jpeg_decode_entropy: %d x %d MCUs, outside [1, %d]", mcu_rows, mcu_cols, A2P_JPEG_MAX_SIZE / 8 + 1);
  ARG(jpeg_luma_blocks(blocks_per_mcu), "jpeg_decode_entropy: blocks_per_mcu=%d, need 1 (grayscale), 3 (4:4:4), 4 (4:2:2) or 6 (4:2:0)",
      blocks_per_mcu);
  ARG(restart_interval >= 0 && restart_interval <= 65535, "jpeg_decode_entropy: restart_interval=%d is outside [0, 65535]", restart_interval);
  ARG(selectors >= 0 && selectors <= 0x77, "jpeg_decode_entropy: selectors=%#x, need the DC table of component c in bit c and its AC table in bit 4 + c",
      selectors);
  const int64_t mcus = (int64_t)mcu_rows * mcu_cols, ri = restart_interval ? restart_interval : mcus, intervals = (mcus + ri - 1) / ri;
  ARG(N * intervals <= (int64_t)0x7fffffff * JPEG_WAVE, "jpeg_decode_entropy: N=%lld frames x %lld intervals exceed the grid", (long long)N,
      (long long)intervals);
  ARG((uintptr_t)coef % 2 == 0, "jpeg_decode_entropy: coef must be 2-byte aligned");
  const int64_t coef_bytes = N * mcus * blocks_per_mcu * 128, range_bytes = N * (intervals + 1) * 8;
  const struct { const char* name; const void* ptr; int64_t n; } inputs[] = {{"data", data, data_bytes}, {"ranges", ranges, range_bytes},
      {"restart_status", restart_status, N * 4}, {"tables", tables, JPEG_TABLES * JPEG_TABLE_WORDS * 4}};
  for (const auto& in : inputs) {
    ARG(!jpeg_bytes_overlap(coef, coef_bytes, in.ptr, in.n), "jpeg_decode_entropy: coef must not alias an input (it overlaps %s)", in.name);
    ARG(!jpeg_bytes_overlap(status, N * 4, in.ptr, in.n), "jpeg_decode_entropy: status must not alias an input (it overlaps %s)", in.name);
  }
  ARG(!jpeg_bytes_overlap(coef, coef_bytes, status, N * 4), "jpeg_decode_entropy: coef must not alias status");
  if (N == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(coef, 0, (size_t)coef_bytes, s));        // the kernel stores the non-zero coefficients only
  HIPCHK(hipMemsetAsync(status, 0, (size_t)N * 4, s));
  JpegDecodeParams p = {};
  p.data = data, p.data_bytes = data_bytes, p.ranges = ranges, p.restart_status = restart_status, p.tables = tables, p.coef = coef;
  p.status = status, p.N = N, p.intervals = intervals, p.mcus = mcus, p.ri = ri;
  p.scan.bpm = blocks_per_mcu, p.scan.ny = jpeg_luma_blocks(blocks_per_mcu);
  for (int c = 0; c < 3; ++c) p.scan.dc[c] = (selectors >> c) & 1, p.scan.ac[c] = (selectors >> (4 + c)) & 1;
  jpeg_decode_kernel<<<(unsigned)((N * intervals + JPEG_WAVE - 1) / JPEG_WAVE), JPEG_WAVE, 0, s>>>(p);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_jpeg_pixels(const int16_t* coef, int64_t N, int32_t H, int32_t W, int32_t components, int32_t luma_h, int32_t luma_v,
                               const uint16_t* qtab, uint8_t* out, int64_t frame_stride, int64_t row_stride, void* stream) {
  ARG(coef && qtab && out, "jpeg_pixels: null coef, qtab or out");
  ARG(N >= 0, "jpeg_pixels: N=%lld is negative", (long long)N);
  ARG(H >= 1 && H <= A2P_JPEG_MAX_SIZE && W >= 1 && W <= A2P_JPEG_MAX_SIZE, "jpeg_pixels: the frames are %d x %d, outside [1, %d]", H, W,
      A2P_JPEG_MAX_SIZE);
  const bool gray = components == 1 && luma_h == 1 && luma_v == 1;
  ARG(gray || (components == 3 && ((luma_h == 1 && luma_v == 1) || (luma_h == 2 && luma_v == 1) || (luma_h == 2 && luma_v == 2))),
      "jpeg_pixels: %d components with luminance sampled %d x %d: need 3 components with 1 x 1 (4:4:4), 2 x 1 (4:2:2) or 2 x 2 (4:2:0) "
      "over 1 x 1 chrominance, or 1 component", components, luma_h, luma_v);
  ARG(row_stride >= (int64_t)3 * W, "jpeg_pixels: row_stride=%lld bytes is below 3 W = %d", (long long)row_stride, 3 * W);
  const int64_t frame = (int64_t)(H - 1) * row_stride + (int64_t)3 * W;
  ARG(frame_stride >= frame || N <= 1, "jpeg_pixels: frame_stride=%lld bytes is below (H - 1) row_stride + 3 W = %lld", (long long)frame_stride,
      (long long)frame);
  ARG((uintptr_t)coef % 4 == 0, "jpeg_pixels: coef must be 4-byte aligned");
  const int mw = 8 * luma_h, mh = 8 * luma_v, bpm = gray ? 1 : luma_h * luma_v + 2, mps = JPEG_DEC_STRIP_PX / mw;
  JpegPixelParams p = {};
  p.mcu_rows = (H + mh - 1) / mh, p.mcu_cols = (W + mw - 1) / mw, p.strips = (p.mcu_cols + mps - 1) / mps;
  ARG(N * p.mcu_rows * p.strips <= 0x7fffffff, "jpeg_pixels: N=%lld frames x %d MCU rows x %d strips exceed the grid", (long long)N,
      p.mcu_rows, p.strips);
  const int64_t coef_bytes = N * p.mcu_rows * p.mcu_cols * bpm * 128, out_bytes = N > 0 ? (N - 1) * frame_stride + frame : 0;
  ARG(!jpeg_bytes_overlap(out, out_bytes, coef, coef_bytes), "jpeg_pixels: out must not alias an input (it overlaps coef)");
  ARG(!jpeg_bytes_overlap(out, out_bytes, qtab, components * 128), "jpeg_pixels: out must not alias an input (it overlaps qtab)");
  if (N == 0) return 0;
  p.coef = coef, p.qtab = qtab, p.out = out, p.frame_stride = frame_stride, p.row_stride = row_stride, p.H = H, p.W = W;
  const unsigned grid = (unsigned)(N * p.mcu_rows * p.strips);
  hipStream_t s = (hipStream_t)stream;
  if (gray) jpeg_pixels_kernel<1, 1, true><<<grid, JPEG_THREADS, 0, s>>>(p);
  else if (luma_v == 2) jpeg_pixels_kernel<2, 2, false><<<grid, JPEG_THREADS, 0, s>>>(p);
  else if (luma_h == 2) jpeg_pixels_kernel<2, 1, false><<<grid, JPEG_THREADS, 0, s>>>(p);
  else jpeg_pixels_kernel<1, 1, false><<<grid, JPEG_THREADS, 0, s>>>(p);
  HIPCHK(hipGetLastError());
  return 0;
}
