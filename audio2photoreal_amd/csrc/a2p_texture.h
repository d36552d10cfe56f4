// C ABI of the texture layers (include/a2p_hip.h "texture layers"; kernels in kernels_texture.h).  Context-free like the decoder
// layers: weights, biases and maps are device arrays the caller prepared once (audio2photoreal_amd/texture.py folds and validates
// them on the host).  Included at the end of a2p_lib.hip after a2p_conv.h (set_err / ARG / HIPCHK / conv_overlap).
#pragma once

// Tile and channel chunk of a strided layer from its shape alone (never from N): planes up to 16 x 16 (counted on the side the
// threads map to: the output of the down layer, the source of the transposed one) take the 8 x 8 tile with four channel groups
// per block, larger ones the 8 x 32 tile; four channels per thread up to C_out = 4, else eight.
struct TexLaunch {
  bool small;
  int co_t, chunk, chunks;     // chunk = channels per block
};

static TexLaunch tex_launch(int32_t rows, int32_t cols, int32_t C_out) {
  TexLaunch l;
  l.small = rows <= 16 && cols <= 16;
  l.co_t = C_out <= 4 ? 4 : 8;
  l.chunk = l.co_t * (l.small ? 4 : 1);
  l.chunks = (C_out + l.chunk - 1) / l.chunk;
  return l;
}

// The checks the two strided layers share; fills the kernel's parameters.  `what` is the entry point's name in messages.
static int tex_conv_setup(const char* what, const a2p_tex_conv_desc* d, bool transposed, TexConvParams* p, TexLaunch* launch) {
  static_assert(TEX_ACT_NONE == A2P_TEX_ACT_NONE && TEX_ACT_LRELU == A2P_TEX_ACT_LRELU && TEX_ACT_SIGMOID == A2P_TEX_ACT_SIGMOID,
                "texture layer activations");
  ARG(d, "%s: null descriptor", what);
  ARG(d->x.data && d->weight && d->out, "%s: null x.data, weight or out", what);
  ARG(d->N >= 0, "%s: N=%lld is negative", what, (long long)d->N);
  ARG(d->x.C >= 1 && d->x.C <= A2P_CONV_MAX_CHANNELS, "%s: x.C=%d, outside [1, %d]", what, d->x.C, A2P_CONV_MAX_CHANNELS);
  ARG(d->C_out >= 1 && d->C_out <= A2P_CONV_MAX_CHANNELS, "%s: C_out=%d, outside [1, %d]", what, d->C_out, A2P_CONV_MAX_CHANNELS);
  const int32_t lo = transposed ? 1 : 2, hi = transposed ? A2P_CONV_MAX_SIZE / 2 : A2P_CONV_MAX_SIZE;
  ARG(d->x.H >= lo && d->x.H <= hi && d->x.W >= lo && d->x.W <= hi, "%s: x is %d x %d, outside [%d, %d]", what, d->x.H, d->x.W, lo, hi);
  const int64_t frame = (int64_t)d->x.C * d->x.H * d->x.W;
  ARG(d->x.frame_stride >= frame, "%s: x.frame_stride=%lld is below C H W = %lld", what, (long long)d->x.frame_stride, (long long)frame);
  ARG(d->bias_mode >= A2P_CONV_BIAS_NONE && d->bias_mode <= A2P_CONV_BIAS_UNTIED, "%s: bias_mode=%d outside [0, 2]", what, d->bias_mode);
  ARG(d->bias_mode == A2P_CONV_BIAS_NONE || d->bias, "%s: bias_mode=%d needs a bias", what, d->bias_mode);
  ARG(d->act >= A2P_TEX_ACT_NONE && d->act <= (transposed ? A2P_TEX_ACT_SIGMOID : A2P_TEX_ACT_LRELU), "%s: act=%d outside [0, %d]", what,
      d->act, transposed ? A2P_TEX_ACT_SIGMOID : A2P_TEX_ACT_LRELU);
  ARG(transposed || !d->skip, "%s: the down layer takes no skip", what);

  p->Hs = d->x.H;
  p->Ws = d->x.W;
  p->H = transposed ? 2 * d->x.H : (d->x.H - 2) / 2 + 1;
  p->W = transposed ? 2 * d->x.W : (d->x.W - 2) / 2 + 1;
  *launch = tex_launch(transposed ? p->Hs : p->H, transposed ? p->Ws : p->W, d->C_out);
  const int th = 8, tw = launch->small ? 8 : 32, rows = transposed ? p->Hs : p->H, cols = transposed ? p->Ws : p->W;
  p->tiles_x = (cols + tw - 1) / tw;
  p->tiles = p->tiles_x * ((rows + th - 1) / th);
  ARG(d->N * p->tiles <= 0x7fffffff, "%s: N=%lld frames x %d tiles exceed the grid", what, (long long)d->N, p->tiles);
  ARG(launch->chunks <= 65535, "%s: %d channel chunks exceed the grid", what, launch->chunks);

  const int64_t HW = (int64_t)p->H * p->W, out_n = d->N * d->C_out * HW;
  const struct { const char* name; const void* ptr; int64_t n; } inputs[] = {
      {"x", d->x.data, d->N > 0 ? (d->N - 1) * d->x.frame_stride + frame : 0},
      {"weight", d->weight, (int64_t)d->C_out * d->x.C * 16},
      {"bias", d->bias_mode ? d->bias : nullptr, d->bias_mode == A2P_CONV_BIAS_UNTIED ? d->C_out * HW : d->C_out},
      {"skip", d->skip, out_n}};
  for (const auto& in : inputs)
    ARG(!conv_overlap(d->out, out_n, in.ptr, in.n), "%s: out must not alias an input (it overlaps %s)", what, in.name);

  p->x = d->x.data;
  p->n_stride = d->x.frame_stride;
  p->w = d->weight;
  p->bias = d->bias_mode ? d->bias : nullptr;
  p->skip = d->skip;
  p->out = d->out;
  p->C_in = d->x.C;
  p->C_out = d->C_out;
  p->bias_mode = d->bias_mode;
  p->act = d->act;
  p->slope = d->slope;
  p->beta = d->beta;
  return 0;
}

extern "C" int a2p_conv2d_down_ub(const a2p_tex_conv_desc* d, void* stream) {
  TexConvParams p = {};
  TexLaunch l;
  if (int rc = tex_conv_setup("conv2d_down_ub", d, false, &p, &l)) return rc;
  if (d->N == 0) return 0;
  const dim3 grid((unsigned)(d->N * p.tiles), (unsigned)l.chunks);
  hipStream_t s = (hipStream_t)stream;
  if (l.small && l.co_t == 8) conv2d_down_kernel<8, 8, 8, 8><<<grid, TEX_THREADS, 0, s>>>(p);
  else if (l.small) conv2d_down_kernel<8, 8, 4, 8><<<grid, TEX_THREADS, 0, s>>>(p);
  else if (l.co_t == 8) conv2d_down_kernel<8, 32, 8, 4><<<grid, TEX_THREADS, 0, s>>>(p);
  else conv2d_down_kernel<8, 32, 4, 4><<<grid, TEX_THREADS, 0, s>>>(p);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_conv_transpose2d_ub(const a2p_tex_conv_desc* d, void* stream) {
  TexConvParams p = {};
  TexLaunch l;
  if (int rc = tex_conv_setup("conv_transpose2d_ub", d, true, &p, &l)) return rc;
  if (d->N == 0) return 0;
  const dim3 grid((unsigned)(d->N * p.tiles), (unsigned)l.chunks);
  hipStream_t s = (hipStream_t)stream;
  if (l.small && l.co_t == 8) conv_transpose2d_kernel<8, 8, 8, 16><<<grid, TEX_THREADS, 0, s>>>(p);
  else if (l.small) conv_transpose2d_kernel<8, 8, 4, 16><<<grid, TEX_THREADS, 0, s>>>(p);
  else if (l.co_t == 8) conv_transpose2d_kernel<8, 32, 8, 8><<<grid, TEX_THREADS, 0, s>>>(p);
  else conv_transpose2d_kernel<8, 32, 4, 8><<<grid, TEX_THREADS, 0, s>>>(p);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_resize_bilinear(const float* x, int64_t planes, int32_t Hs, int32_t Ws, int32_t H, int32_t W, float* out, void* stream) {
  ARG(x && out, "resize_bilinear: null argument");
  ARG(planes >= 0, "resize_bilinear: planes=%lld is negative", (long long)planes);
  ARG(Hs >= 1 && Hs <= A2P_CONV_MAX_SIZE && Ws >= 1 && Ws <= A2P_CONV_MAX_SIZE, "resize_bilinear: the source is %d x %d, outside [1, %d]", Hs,
      Ws, A2P_CONV_MAX_SIZE);
  ARG(H >= 1 && H <= A2P_CONV_MAX_SIZE && W >= 1 && W <= A2P_CONV_MAX_SIZE, "resize_bilinear: the output is %d x %d, outside [1, %d]", H, W,
      A2P_CONV_MAX_SIZE);
  const int64_t HW = (int64_t)H * W, bpp = (HW + TEX_THREADS - 1) / TEX_THREADS;
  ARG(planes * bpp <= 0x7fffffff, "resize_bilinear: %lld planes of %d x %d exceed the grid", (long long)planes, H, W);
  ARG(!conv_overlap(out, planes * HW, x, planes * Hs * Ws), "resize_bilinear: out must not alias x");
  if (planes == 0) return 0;
  resize_bilinear_kernel<<<(unsigned)(planes * bpp), TEX_THREADS, 0, (hipStream_t)stream>>>(x, Hs, Ws, H, W, (float)Hs / (float)H,
                                                                                          (float)Ws / (float)W, (unsigned)bpp, out);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_texture_compose(const float* t, const float* u, const float* tex_mean, float tex_std, const float* shadow,
                                   int32_t shadow_frames, int64_t N, int32_t C, int32_t Sh, int32_t Sw, float* out, void* stream) {
  ARG(t && u && tex_mean && out, "texture_compose: null t, u, tex_mean or out");
  ARG(N >= 0, "texture_compose: N=%lld is negative", (long long)N);
  ARG(C >= 1 && 4 * C <= A2P_CONV_MAX_CHANNELS, "texture_compose: C=%d, outside [1, %d]", C, A2P_CONV_MAX_CHANNELS / 4);
  ARG(Sh >= 1 && Sh <= A2P_CONV_MAX_SIZE / 2 && Sw >= 1 && Sw <= A2P_CONV_MAX_SIZE / 2, "texture_compose: t is %d x %d, outside [1, %d]", Sh, Sw,
      A2P_CONV_MAX_SIZE / 2);
  ARG(!shadow || shadow_frames == 1 || shadow_frames == N, "texture_compose: shadow holds %d frames, need 1 or N=%lld", shadow_frames,
      (long long)N);
  const int64_t S = (int64_t)Sh * Sw, out_n = N * C * 4 * S, bpp = (S + TEX_THREADS - 1) / TEX_THREADS;
  ARG(N * C * bpp <= 0x7fffffff, "texture_compose: N=%lld x C=%d maps of %d x %d exceed the grid", (long long)N, C, Sh, Sw);
  const struct { const char* name; const void* ptr; int64_t n; } inputs[] = {
      {"t", t, N * C * S}, {"u", u, N * 4 * C * S}, {"tex_mean", tex_mean, C * 4 * S}, {"shadow", shadow, shadow_frames * 4 * S}};
  for (const auto& in : inputs)
    ARG(!conv_overlap(out, out_n, in.ptr, in.n), "texture_compose: out must not alias an input (it overlaps %s)", in.name);
  if (N == 0) return 0;
  texture_compose_kernel<<<(unsigned)(N * C * bpp), TEX_THREADS, 0, (hipStream_t)stream>>>(t, u, tex_mean, tex_std, shadow,
                                                                                         shadow && shadow_frames > 1 ? 4 * S : 0, C, Sh, Sw,
                                                                                         (unsigned)bpp, out);
  HIPCHK(hipGetLastError());
  return 0;
}
