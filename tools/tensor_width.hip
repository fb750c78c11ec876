// tools/tensor_width.hip -- tensor_kernel's one-word-per-lane form against a two-words-per-lane (16-byte) form and a 16-byte copy, same buffers
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <vector>
#include "ntt_ct_mul.h"
using namespace ntt;
#define CK(x) do { hipError_t e_ = (x); if(e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while(0)
struct K { uint64_t *c[3]; const uint64_t *a[2], *b[2]; int square; uint64_t limb_stride, poly_stride, batch; uint32_t logn; BconvDst ql[16]; };
__device__ __forceinline__ void one(uint64_t x0, uint64_t x1, uint64_t y0, uint64_t y1, const BconvDst &d, uint64_t &r0, uint64_t &r1, uint64_t &r2)
{
  uint64_t h1 = 0, l1 = 0;
  bconv_mac(h1, l1, x0, y1);
  bconv_mac(h1, l1, x1, y0);
  const uint64_t v0 = bconv_reduce(mulhi64(x0, y0), x0 * y0, d), v1 = bconv_reduce(h1, l1, d), v2 = bconv_reduce(mulhi64(x1, y1), x1 * y1, d);
  r0 = v0 >= d.q ? v0 - d.q : v0; r1 = v1 >= d.q ? v1 - d.q : v1; r2 = v2 >= d.q ? v2 - d.q : v2;
}
__global__ void __launch_bounds__(256) t8(const K k)
{
  const BconvDst d = k.ql[blockIdx.y];
  const uint64_t lo = (uint64_t)blockIdx.y * k.limb_stride, n = k.batch << k.logn;
  const uint32_t mask = (1u << k.logn) - 1u;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t at = lo + (i >> k.logn) * k.poly_stride + ((uint32_t)i & mask);
    const uint64_t x0 = k.a[0][at], x1 = k.a[1][at], y0 = k.square ? x0 : k.b[0][at], y1 = k.square ? x1 : k.b[1][at];
    uint64_t r0, r1, r2;
    one(x0, x1, y0, y1, d, r0, r1, r2);
    k.c[0][at] = r0; k.c[1][at] = r1; k.c[2][at] = r2;
  }
}
__global__ void __launch_bounds__(256) t16(const K k)
{
  const BconvDst d = k.ql[blockIdx.y];
  const uint64_t lo = (uint64_t)blockIdx.y * k.limb_stride, n2 = (k.batch << k.logn) >> 1;
  const uint32_t mask = (1u << k.logn) - 1u;
  for(uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n2; j += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = 2 * j, at = lo + (i >> k.logn) * k.poly_stride + ((uint32_t)i & mask);
    const ulonglong2 x0 = *(const ulonglong2 *)(k.a[0] + at), x1 = *(const ulonglong2 *)(k.a[1] + at);
    const ulonglong2 y0 = k.square ? x0 : *(const ulonglong2 *)(k.b[0] + at), y1 = k.square ? x1 : *(const ulonglong2 *)(k.b[1] + at);
    uint64_t r0, r1, r2, s0, s1, s2;
    one(x0.x, x1.x, y0.x, y1.x, d, r0, r1, r2);
    one(x0.y, x1.y, y0.y, y1.y, d, s0, s1, s2);
    *(ulonglong2 *)(k.c[0] + at) = make_ulonglong2(r0, s0); *(ulonglong2 *)(k.c[1] + at) = make_ulonglong2(r1, s1); *(ulonglong2 *)(k.c[2] + at) = make_ulonglong2(r2, s2);
  }
}
__global__ void __launch_bounds__(256) cp16(ulonglong2 *dst, const ulonglong2 *src, uint64_t n2)
{
  for(uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n2; j += (uint64_t)gridDim.x * blockDim.x) dst[j] = src[j];
}
__global__ void fill(uint64_t *a, uint64_t n, uint64_t q, uint64_t seed)
{
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) a[i] = ((i + seed) * 0x9E3779B97F4A7C15ull) % q;
}
int main(int argc, char **argv)
{
  const uint32_t logn = argc > 1 ? atoi(argv[1]) : 14;
  const uint64_t batch = argc > 2 ? strtoull(argv[2], 0, 0) : 1024;
  const int NL = 24, REP = 10, WIN = 5;
  const uint64_t N = 1ull << logn, words = (uint64_t)NL * batch * N, q = 1125899906826241ull; /* a 50-bit odd modulus: timing only */
  uint64_t *buf[7];
  for(int i = 0; i < 7; i++) { CK(hipMalloc(&buf[i], words * 8)); hipLaunchKernelGGL(fill, dim3(4096), dim3(256), 0, 0, buf[i], words, q, 1000 * i); }
  CK(hipDeviceSynchronize());
  BconvDst d{}; d.q = q; d.bar = ~0ull / q; const unsigned __int128 mu = ~(unsigned __int128)0 / q; d.mu_lo = (uint64_t)mu; d.mu_hi = (uint64_t)(mu >> 64);
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const uint64_t n = batch << logn;
  auto run = [&](int which, int square) {
    for(int f = 0; f < NL; f += 16) {
      K k{}; const int nl = std::min(16, NL - f);
      for(int j = 0; j < 3; j++) k.c[j] = buf[4 + j] + (uint64_t)f * batch * N;
      for(int j = 0; j < 2; j++) { k.a[j] = buf[j] + (uint64_t)f * batch * N; k.b[j] = buf[(square ? 0 : 2) + j] + (uint64_t)f * batch * N; }
      k.square = square; k.limb_stride = batch * N; k.poly_stride = N; k.batch = batch; k.logn = logn;
      for(int l = 0; l < nl; l++) k.ql[l] = d;
      if(which == 8) hipLaunchKernelGGL(t8, dim3(coef_grid(n, 0), nl), dim3(256), 0, 0, k);
      else hipLaunchKernelGGL(t16, dim3(coef_grid(n / 2, 0), nl), dim3(256), 0, 0, k);
    }
  };
  auto copy = [&]() { hipLaunchKernelGGL(cp16, dim3(coef_grid(words / 2, 0)), dim3(256), 0, 0, (ulonglong2 *)buf[4], (const ulonglong2 *)buf[0], words / 2); };
  struct V { const char *name; int which, square; } vs[] = {{"copy16", 0, 0}, {"tensor8", 8, 0}, {"tensor16", 16, 0}, {"square8", 8, 1}, {"square16", 16, 1}};
  std::vector<float> ms[5];
  for(int w = 0; w < WIN + 1; w++)
    for(int v = 0; v < 5; v++) {
      CK(hipEventRecord(e0, 0));
      for(int r = 0; r < REP; r++) { if(vs[v].which) run(vs[v].which, vs[v].square); else copy(); }
      CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
      float t; CK(hipEventElapsedTime(&t, e0, e1));
      if(w) ms[v].push_back(t / REP); /* the first window warms up */
    }
  for(int v = 0; v < 5; v++) { std::sort(ms[v].begin(), ms[v].end()); printf("N=2^%u polys=%llu %-9s median %8.4f ms  min %8.4f  max %8.4f  / copy16 %.2f\n", logn, (unsigned long long)batch, vs[v].name, ms[v][WIN / 2], ms[v].front(), ms[v].back(), ms[v][WIN / 2] / ms[0][WIN / 2]); }
  /* the two forms agree */
  run(8, 0); CK(hipDeviceSynchronize());
  std::vector<uint64_t> h8(3 * 4096), h16(3 * 4096);
  for(int j = 0; j < 3; j++) CK(hipMemcpy(h8.data() + 4096 * j, buf[4 + j] + words - 4096, 4096 * 8, hipMemcpyDeviceToHost));
  run(16, 0); CK(hipDeviceSynchronize());
  for(int j = 0; j < 3; j++) CK(hipMemcpy(h16.data() + 4096 * j, buf[4 + j] + words - 4096, 4096 * 8, hipMemcpyDeviceToHost));
  printf("forms agree on the last 4096 words: %s\n", h8 == h16 ? "yes" : "NO");
  return 0;
}
