/* slots.hip -- the element-wise kernels of the BFV / BGV slot encode and decode (ntt_slots.h states the order):
 *   slots_table_kernel  a plan's pos / ipos tables on the device (ntt_plan_enable_slots), one thread per slot;
 *   slots_perm_kernel   out[p][s] = in[p][tab[s]]: the composition's half of ntt_slots_encode_batch (tab = ipos, in front of the
 *                       inverse transform) and of ntt_slots_decode_batch (tab = pos, behind the forward transform).  16N bytes per
 *                       polynomial and the 4N-byte table, which the batch shares.  Words are copied bit for bit: every policy, N >= 2. */
#include "ntt_slots.h"

namespace ntt {

__global__ void __launch_bounds__(256) slots_table_kernel(uint32_t *pos, uint32_t *ipos, uint32_t logn)
{
  const uint64_t n = 1ull << logn;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t p = (uint32_t)slot_position(logn, i); /* below n: a bit reversal of m bits */
    pos[i]           = p;
    ipos[p]          = (uint32_t)i; /* pos is a permutation: every word of ipos is written once */
  }
}

hipError_t launch_slots_tables(uint32_t *pos, uint32_t *ipos, uint32_t logn, hipStream_t stream)
{
  if(!pos || !ipos || logn < 1 || logn > 28) return hipErrorInvalidValue;
  hipLaunchKernelGGL(slots_table_kernel, dim3(coef_grid(1ull << logn, 0)), dim3(256), 0, stream, pos, ipos, logn);
  return hipGetLastError();
}

struct KSlotsPerm {
  uint64_t *      out;
  const uint64_t *in;
  const uint32_t *tab;
  uint64_t        out_stride, in_stride, batch;
  uint32_t        logn;
};

/* one word per thread and iteration (galois_ntt_kernel's shape): the store is coalesced, the load gathered inside the polynomial */
__global__ void __launch_bounds__(256) slots_perm_kernel(const KSlotsPerm k)
{
  const uint64_t n    = k.batch << k.logn;
  const uint64_t mask = (1ull << k.logn) - 1ull;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p = i >> k.logn, s = i & mask;
    k.out[p * k.out_stride + s] = k.in[p * k.in_stride + (k.tab[s] & mask)]; /* (the mask: no table word leaves the polynomial) */
  }
}

hipError_t launch_slots_perm(const SlotsPermArgs &sa)
{
  if(sa.logn < 1 || sa.logn > 28 || !sa.tab) return hipErrorInvalidValue;
  const uint64_t N = 1ull << sa.logn;
  KSlotsPerm     k{};
  k.out        = sa.out;
  k.in         = sa.in;
  k.tab        = sa.tab;
  k.out_stride = sa.out_stride ? sa.out_stride : N;
  k.in_stride  = sa.in_stride ? sa.in_stride : N;
  k.batch      = sa.batch;
  k.logn       = sa.logn;
  const uint64_t n = sa.batch << sa.logn;
  if(n == 0) return hipSuccess;
  hipLaunchKernelGGL(slots_perm_kernel, dim3(coef_grid(n, sa.max_grid)), dim3(256), 0, sa.stream, k);
  return hipGetLastError();
}

} /* namespace ntt */
