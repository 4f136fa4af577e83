// division_magic_main.cpp -- host check of division_magic (csrc/tiled_scatter.h): the quotient the LDS-tile scatter
// computes for a table entry e, umulhi(e, magic) >> shift, is e / K for every dividend below 2^31.  A wrong quotient
// would send an addend to the wrong query row without any error.  Launches no kernel; needs no GPU.
//
// Checked: every K in 1..4096 and 2000 sampled K up to 2^31 - 1; for each, e in {0, 1, qK - 1, qK, qK + 1} for sampled
// q and for the largest q with qK < 2^31, and e = 2^31 - 1.  Prints the first mismatch and exits non-zero.
#include <cstdint>
#include <cstdio>

#include "../../pytorch3d_pointops_amd/csrc/tiled_scatter.h"

namespace {

constexpr uint64_t kLimit = 1ull << 31;  // dividends are below this

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t next_u64() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// what the kernel computes: __umulhi(e, magic) >> shift, or e itself for K = 1 (shift = -1)
uint32_t kernel_quotient(uint32_t e, pointops::DivMagic dm) {
  if (dm.shift < 0) return e;
  return (uint32_t)((((uint64_t)e * dm.magic) >> 32) >> dm.shift);
}

long checked = 0;

bool check(uint32_t K, pointops::DivMagic dm, uint64_t e) {
  if (e >= kLimit) return true;
  ++checked;
  const uint32_t got = kernel_quotient((uint32_t)e, dm), want = (uint32_t)e / K;
  if (got == want) return true;
  printf("MISMATCH K=%u e=%llu: umulhi(e, %u) >> %d = %u, e / K = %u\n", K, (unsigned long long)e, dm.magic, dm.shift,
         got, want);
  return false;
}

bool check_divisor(uint32_t K) {
  const pointops::DivMagic dm = pointops::division_magic(K);
  if ((K == 1) != (dm.shift < 0)) {
    printf("MISMATCH K=%u: shift = %d\n", K, dm.shift);
    return false;
  }
  bool ok = check(K, dm, 0) && check(K, dm, 1) && check(K, dm, kLimit - 1);
  const uint64_t qmax = (kLimit - 1) / K;  // the largest q with q K < 2^31
  const uint64_t qs[] = {1, 2, qmax, qmax > 0 ? qmax - 1 : 0, qmax / 2 + 1};
  for (uint64_t q : qs) ok = ok && check(K, dm, q * K - (q > 0)) && check(K, dm, q * K) && check(K, dm, q * K + 1);
  for (int s = 0; ok && s < 64; ++s) {
    const uint64_t q = next_u64() % (qmax + 1);
    ok = check(K, dm, q * K + K - 1) && check(K, dm, q * K) && check(K, dm, q * K + 1) &&
         (q == 0 || check(K, dm, q * K - 1));
  }
  return ok;
}

}  // namespace

int main() {
  for (uint32_t K = 1; K <= 4096; ++K)
    if (!check_divisor(K)) return 1;
  const uint32_t edges[] = {4097, 65535, 65536, 65537, (1u << 30) - 1, 1u << 30, (1u << 30) + 1, (1u << 31) - 2,
                            (1u << 31) - 1};
  for (uint32_t K : edges)
    if (!check_divisor(K)) return 1;
  for (int s = 0; s < 2000; ++s) {
    // half of the samples uniform in [4097, 2^31), half with a uniform bit length (small divisors have the long quotients)
    uint32_t K = (uint32_t)(next_u64() % (kLimit - 4097)) + 4097;
    if (s & 1) K = (K >> (next_u64() % 19)) | 4097u;
    if (!check_divisor(K)) return 1;
  }
  printf("division_magic: %ld dividends checked, no mismatch\n", checked);
  return 0;
}
