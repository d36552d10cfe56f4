// Occupancy / balance probe of the attention kernel (scratch; not product): the same kernel with grids that give every CU exactly
// 1, 2, 2.5, 3, 4, 6 workgroups -- is a CU's throughput saturated at 2 resident workgroups (then the 640-workgroup launch of the
// headline, 2.5 per CU, loses 17 % to imbalance) or does it still scale (then it is latency-bound and balance does not matter)?
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../audio2photoreal_amd/csrc/kernels_attn.h"
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)
template <typename F>
float time_it(F f, int iters = 20) {
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int i = 0; i < 3; ++i) f();
  CK(hipEventRecord(e0)); for (int i = 0; i < iters; ++i) f(); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
  float ms; CK(hipEventElapsedTime(&ms, e0, e1)); return ms / iters * 1e3f;
}
template <int DH> void sweep(int nseq, int S) {
  const int d = 8 * DH, Tmax = 1536;
  const int Sld = (S + 63) / 64 * 64;
  h16_t *q, *k, *vt, *o;
  CK(hipMalloc(&q, (size_t)nseq * Tmax * d * 2)); CK(hipMalloc(&k, ((size_t)nseq * Sld + 64) * d * 2));
  CK(hipMalloc(&vt, (size_t)nseq * d * Sld * 2)); CK(hipMalloc(&o, (size_t)nseq * Tmax * d * 2));
  std::vector<uint16_t> h((size_t)nseq * (Sld > Tmax ? Sld : Tmax) * d + 64 * d);
  for (auto& v : h) v = 0x3800 + (rand() & 0x7ff) - ((rand() & 1) << 15);
  CK(hipMemcpy(k, h.data(), ((size_t)nseq * Sld + 64) * d * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(vt, h.data(), (size_t)nseq * d * Sld * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(q, h.data(), (size_t)nseq * Tmax * d * 2, hipMemcpyHostToDevice));
  printf("dh=%d nseq=%d S=%d: workgroups per CU -> us per launch, us per (workgroup per CU)\n", DH, nseq, S);
  const int pairs = nseq * 8;
  for (int T : {128 * 256 / pairs, 128 * 512 / pairs, 600, 128 * 768 / pairs, 128 * 1024 / pairs, 128 * 1536 / pairs, 128 * 2304 / pairs, 128 * 3072 / pairs}) {
    if (T < 128 || T > Tmax) continue;
    AttnP a; memset(&a, 0, sizeof(a));
    a.Q = q; a.q_seq_stride = (int64_t)T * d; a.ldq = d; a.K = k; a.k_slot_stride = (int64_t)Sld * d; a.ldk = d;
    a.VT = vt; a.vt_slot_stride = (int64_t)d * Sld; a.ldvt = Sld; a.O = o; a.o_seq_stride = (int64_t)T * d; a.ldo = d;
    a.tail_mod = 1; a.Tq = T; a.S_main = S; a.S_tail = 0; a.scale_log2e = 1.4426950408889634f / sqrtf((float)DH);
    a.nq = (T + 127) / 128; a.nheads = 8; a.nseq = nseq; a.xcd_remap = 1;
    dim3 grid(a.nq * 8 * nseq);
    float us = time_it([&] { attn_kernel<h16_t, DH><<<grid, 256>>>(a); });
    CK(hipDeviceSynchronize());
    const double wpc = grid.x / 256.0;
    const double gf = 4.0 * nseq * 8 * (double)T * S * DH * 1e-9;
    printf("  T=%5d grid=%5d  %.2f per CU  %8.1f us  %6.1f us/(wg/CU)  %7.1f TF\n", T, grid.x, wpc, us, us / wpc, gf / us * 1e3);
  }
  CK(hipFree(q)); CK(hipFree(k)); CK(hipFree(vt)); CK(hipFree(o));
}
// (The 64-queries-per-wave and key-split comparisons needed patched kernel headers (attn_keysplit_experiment.patch); their code is in the
// history up to commit 21066ce, their results in profiles/r04_attn_occupancy_probe.txt.)
int main() {
  sweep<64>(16, 2000);
  sweep<64>(16, 600);
  sweep<32>(32, 2000);
  sweep<32>(32, 600);
  return 0;
}
