// C ABI of the encode layers (include/a2p_hip.h "encode layers"; kernels in kernels_encode.h).  Context-free like the decoder and
// texture layers: weights, biases, masks and skinning tables are device arrays the caller prepared once (audio2photoreal_amd/
// encoder.py and skinning.py fold and validate them on the host).  Included at the end of a2p_lib.hip after a2p_texture.h
// (set_err / ARG / HIPCHK / conv_overlap / tex_launch).
#pragma once

extern "C" int a2p_linear_f32(const float* x, int64_t ldx, const float* weight, const float* bias, int64_t N, int32_t I, int32_t O,
                              int32_t act, float slope, float* out, int64_t ldo, float* scratch, int64_t scratch_floats, void* stream) {
  static_assert(LIN_KSLICE == A2P_LINEAR_KSLICE, "linear layer slice");
  ARG(x && weight && out, "linear_f32: null x, weight or out");
  ARG(N >= 0, "linear_f32: N=%lld is negative", (long long)N);
  ARG(I >= 1 && O >= 1, "linear_f32: I=%d, O=%d: both must be >= 1", I, O);
  ARG(ldx >= I && ldo >= O, "linear_f32: ldx=%lld, ldo=%lld are below I=%d, O=%d", (long long)ldx, (long long)ldo, I, O);
  ARG(act == 0 || act == 1, "linear_f32: act=%d, need 0 (none) or 1 (LeakyReLU)", act);
  const int S = (I + LIN_KSLICE - 1) / LIN_KSLICE;            // from I alone: a frame's bits must not depend on N
  const int64_t row_blocks = (N + LIN_ROWS - 1) / LIN_ROWS, need = S > 1 ? (int64_t)S * N * O : 0;
  ARG(S <= 65535 && row_blocks <= 65535, "linear_f32: %d slices x %lld row blocks exceed the grid", S, (long long)row_blocks);
  ARG((N * O + LIN_THREADS - 1) / LIN_THREADS <= 0x7fffffff, "linear_f32: N=%lld x O=%d exceed the grid", (long long)N, O);
  ARG(need == 0 || (scratch && scratch_floats >= need), "linear_f32: I=%d takes %d slices: scratch must hold %lld floats (got %lld)", I, S,
      (long long)need, (long long)(scratch ? scratch_floats : 0));
  const int64_t x_n = N > 0 ? (N - 1) * ldx + I : 0, out_n = N > 0 ? (N - 1) * ldo + O : 0;
  const struct { const char* name; const void* ptr; int64_t n; } inputs[] = {
      {"x", x, x_n}, {"weight", weight, (int64_t)O * I}, {"bias", bias, O}};
  for (const auto& in : inputs) {
    ARG(!conv_overlap(out, out_n, in.ptr, in.n), "linear_f32: out must not alias an input (it overlaps %s)", in.name);
    ARG(!conv_overlap(scratch, need, in.ptr, in.n), "linear_f32: scratch must not alias an input (it overlaps %s)", in.name);
  }
  ARG(!conv_overlap(out, out_n, scratch, need), "linear_f32: out must not alias scratch");
  if (N == 0) return 0;

  LinearParams p = {};
  p.x = x, p.w = weight, p.bias = bias, p.out = out, p.part = scratch;
  p.N = N, p.ldx = ldx, p.ldo = ldo, p.I = I, p.O = O, p.S = S, p.act = act, p.slope = slope;
  const dim3 grid((unsigned)((O + LIN_OT - 1) / LIN_OT), (unsigned)S, (unsigned)row_blocks);
  hipStream_t s = (hipStream_t)stream;
  // the widest load every weight row start allows; only the loads differ, never the arithmetic
  if (I % 4 == 0 && (uintptr_t)weight % 16 == 0) linear_partial_kernel<4><<<grid, LIN_THREADS, 0, s>>>(p);
  else if (I % 2 == 0 && (uintptr_t)weight % 8 == 0) linear_partial_kernel<2><<<grid, LIN_THREADS, 0, s>>>(p);
  else linear_partial_kernel<1><<<grid, LIN_THREADS, 0, s>>>(p);
  if (S > 1) linear_reduce_kernel<<<(unsigned)((N * O + LIN_THREADS - 1) / LIN_THREADS), LIN_THREADS, 0, s>>>(p);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_conv2d_down3_ub(const a2p_down3_desc* d, void* stream) {
  const char* what = "conv2d_down3_ub";
  ARG(d, "%s: null descriptor", what);
  ARG(d->h.data && d->x.data && d->w2 && d->b2 && d->wr && d->out, "%s: null h.data, x.data, w2, b2, wr or out", what);
  ARG(d->N >= 0, "%s: N=%lld is negative", what, (long long)d->N);
  ARG(d->h.C >= 1 && d->h.C <= A2P_CONV_MAX_CHANNELS, "%s: h.C=%d, outside [1, %d]", what, d->h.C, A2P_CONV_MAX_CHANNELS);
  ARG(d->C_out >= 1 && d->C_out <= A2P_CONV_MAX_CHANNELS, "%s: C_out=%d, outside [1, %d]", what, d->C_out, A2P_CONV_MAX_CHANNELS);
  ARG(d->h.H >= 1 && d->h.H <= A2P_CONV_MAX_SIZE && d->h.W >= 1 && d->h.W <= A2P_CONV_MAX_SIZE, "%s: h is %d x %d, outside [1, %d]", what,
      d->h.H, d->h.W, A2P_CONV_MAX_SIZE);
  ARG(d->x.C == d->h.C && d->x.H == d->h.H && d->x.W == d->h.W, "%s: x is [%d, %d, %d], h [%d, %d, %d]: they must agree", what, d->x.C,
      d->x.H, d->x.W, d->h.C, d->h.H, d->h.W);
  const int64_t frame = (int64_t)d->h.C * d->h.H * d->h.W;
  ARG(d->h.frame_stride >= frame && d->x.frame_stride >= frame, "%s: frame strides %lld (h), %lld (x) are below C H W = %lld", what,
      (long long)d->h.frame_stride, (long long)d->x.frame_stride, (long long)frame);

  Down3Params p = {};
  p.Hs = d->h.H, p.Ws = d->h.W;
  p.H = (p.Hs - 1) / 2 + 1, p.W = (p.Ws - 1) / 2 + 1;
  const TexLaunch l = tex_launch(p.H, p.W, d->C_out);
  const int th = 8, tw = l.small ? 8 : 32;
  p.tiles_x = (p.W + tw - 1) / tw;
  p.tiles = p.tiles_x * ((p.H + th - 1) / th);
  ARG(d->N * p.tiles <= 0x7fffffff, "%s: N=%lld frames x %d tiles exceed the grid", what, (long long)d->N, p.tiles);
  ARG(l.chunks <= 65535, "%s: %d channel chunks exceed the grid", what, l.chunks);

  const int64_t HW = (int64_t)p.H * p.W, out_n = d->N * d->C_out * HW;
  const struct { const char* name; const void* ptr; int64_t n; } inputs[] = {
      {"h", d->h.data, d->N > 0 ? (d->N - 1) * d->h.frame_stride + frame : 0},
      {"x", d->x.data, d->N > 0 ? (d->N - 1) * d->x.frame_stride + frame : 0},
      {"w2", d->w2, (int64_t)d->C_out * d->h.C * 9},
      {"b2", d->b2, d->C_out * HW},
      {"wr", d->wr, (int64_t)d->C_out * d->h.C},
      {"br", d->br, d->C_out}};
  for (const auto& in : inputs)
    ARG(!conv_overlap(d->out, out_n, in.ptr, in.n), "%s: out must not alias an input (it overlaps %s)", what, in.name);
  if (d->N == 0) return 0;

  p.h = d->h.data, p.x = d->x.data, p.h_stride = d->h.frame_stride, p.x_stride = d->x.frame_stride;
  p.w2 = d->w2, p.b2 = d->b2, p.wr = d->wr, p.br = d->br, p.out = d->out;
  p.C_in = d->h.C, p.C_out = d->C_out, p.slope = d->slope;
  const dim3 grid((unsigned)(d->N * p.tiles), (unsigned)l.chunks);
  hipStream_t s = (hipStream_t)stream;
  if (l.small && l.co_t == 8) conv2d_down3_kernel<8, 8, 8, 8><<<grid, TEX_THREADS, 0, s>>>(p);
  else if (l.small) conv2d_down3_kernel<8, 8, 4, 8><<<grid, TEX_THREADS, 0, s>>>(p);
  else if (l.co_t == 8) conv2d_down3_kernel<8, 32, 8, 4><<<grid, TEX_THREADS, 0, s>>>(p);
  else conv2d_down3_kernel<8, 32, 4, 4><<<grid, TEX_THREADS, 0, s>>>(p);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_unskin_vertices(const float* mats, int64_t N, int32_t J, const float* verts, const float* tmpl, const int32_t* idx,
                                   const float* w, int32_t V, int32_t K, float gx, float gy, float gz, float* out, void* stream) {
  ARG(mats && verts && tmpl && idx && w && out, "unskin_vertices: null argument");
  ARG(J >= 1 && J <= A2P_SKIN_MAX_JOINTS, "unskin_vertices: J=%d outside [1, %d]", J, A2P_SKIN_MAX_JOINTS);
  ARG(K >= 1 && K <= A2P_SKIN_MAX_INFLUENCES, "unskin_vertices: K=%d outside [1, %d]", K, A2P_SKIN_MAX_INFLUENCES);
  ARG(V >= 1 && (int64_t)V * K <= 0x7fffffff, "unskin_vertices: V=%d, K=%d: need V >= 1 and V K < 2^31", V, K);
  const int tiles = (V + SKIN_VTILE - 1) / SKIN_VTILE;
  ARG(N >= 0 && N * tiles <= 0x7fffffff, "unskin_vertices: N=%lld frames x %d vertex tiles exceed the grid", (long long)N, tiles);
  const int64_t out_n = N * V * 3;
  const struct { const char* name; const void* ptr; int64_t n; } inputs[] = {
      {"mats", mats, N * J * 12}, {"verts", verts, out_n}, {"template", tmpl, (int64_t)V * 3}, {"idx", idx, (int64_t)V * K},
      {"w", w, (int64_t)V * K}};
  for (const auto& in : inputs)
    ARG(!conv_overlap(out, out_n, in.ptr, in.n), "unskin_vertices: out must not alias an input (it overlaps %s)", in.name);
  if (N == 0) return 0;
  const size_t lds = ((size_t)12 * J + 3 * SKIN_THREADS) * sizeof(float);   // <= 51 KiB
  unskin_vertices_kernel<<<(unsigned)(N * tiles), SKIN_THREADS, lds, (hipStream_t)stream>>>(mats, J, verts, tmpl, idx, w, V, K, tiles, gx,
                                                                                          gy, gz, out);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_face_tex_cond(const float* raw, const float* bias, const float* mask, int64_t N, int32_t C, int32_t Hs, int32_t Ws,
                                 int32_t H, int32_t W, float* out, void* stream) {
  ARG(raw && bias && mask && out, "face_tex_cond: null argument");
  ARG(N >= 0, "face_tex_cond: N=%lld is negative", (long long)N);
  ARG(C >= 1 && C <= A2P_CONV_MAX_CHANNELS, "face_tex_cond: C=%d, outside [1, %d]", C, A2P_CONV_MAX_CHANNELS);
  ARG(Hs >= 1 && Hs <= A2P_CONV_MAX_SIZE && Ws >= 1 && Ws <= A2P_CONV_MAX_SIZE, "face_tex_cond: the source is %d x %d, outside [1, %d]", Hs,
      Ws, A2P_CONV_MAX_SIZE);
  ARG(H >= 1 && H <= A2P_CONV_MAX_SIZE && W >= 1 && W <= A2P_CONV_MAX_SIZE, "face_tex_cond: the output is %d x %d, outside [1, %d]", H, W,
      A2P_CONV_MAX_SIZE);
  const int64_t HW = (int64_t)H * W, S = (int64_t)Hs * Ws, bpp = (HW + TEX_THREADS - 1) / TEX_THREADS, out_n = N * C * HW;
  ARG(N * C * bpp <= 0x7fffffff, "face_tex_cond: N=%lld x C=%d planes of %d x %d exceed the grid", (long long)N, C, H, W);
  const struct { const char* name; const void* ptr; int64_t n; } inputs[] = {{"raw", raw, N * C * S}, {"bias", bias, C * S}, {"mask", mask, HW}};
  for (const auto& in : inputs)
    ARG(!conv_overlap(out, out_n, in.ptr, in.n), "face_tex_cond: out must not alias an input (it overlaps %s)", in.name);
  if (N == 0) return 0;
  face_tex_cond_kernel<<<(unsigned)(N * C * bpp), TEX_THREADS, 0, (hipStream_t)stream>>>(raw, bias, mask, C, Hs, Ws, H, W, (float)Hs / (float)H,
                                                                                       (float)Ws / (float)W, (unsigned)bpp, out);
  HIPCHK(hipGetLastError());
  return 0;
}
