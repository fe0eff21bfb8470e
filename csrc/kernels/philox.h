// Philox4x32-10 (Random123's round function) for the counter-based dropout of the streaming
// kernels.  flash_attn.hip keeps its own copy next to the attention keep mask; the two agree, and
// dtg.ops._cpu.philox4x32_10 is the Python side of both.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dtg {
namespace philox {

__device__ __forceinline__ void rounds10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint32_t lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
    const uint32_t lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = lo1;
    c[2] = n2;
    c[3] = lo0;
  }
}

// Key and offset word of one dropout call, from the int64 [2] device tensor {seed, offset} of
// dtg::philox_rng read as four 32-bit words: key = {seed lo, seed hi ^ offset hi}, off = offset lo
// (the offset's high word keys the generator, so offsets past 2^32 never repeat a mask).
struct Key {
  uint32_t k0, k1, off;
};

__device__ __forceinline__ Key load_key(const uint32_t* rng) { return {rng[0], rng[1] ^ rng[3], rng[2]}; }

}  // namespace philox
}  // namespace dtg
