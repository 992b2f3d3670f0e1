// chain_device.hpp -- what chain.hip shares with the other sources of the chain step (crosslink.hip): the counter-based
// generator every reference app draws from, and the per-body sort of a body -> entry incidence.
#pragma once
#include "mhip_internal.hpp"

namespace mhip {

// ---- Philox4x32-10 -----------------------------------------------------------------------------------------------
// counter (c0, c1, c2, c3), key (k0, k1): ten rounds, the key bumped by the Weyl increments between rounds
constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

__device__ inline uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r > 0) {
      k.x += kPhiloxW0;
      k.y += kPhiloxW1;
    }
    const uint64_t p0 = static_cast<uint64_t>(kPhiloxM0) * c.x;
    const uint64_t p1 = static_cast<uint64_t>(kPhiloxM1) * c.z;
    c = make_uint4(static_cast<uint32_t>(p1 >> 32) ^ c.y ^ k.x, static_cast<uint32_t>(p1),
                   static_cast<uint32_t>(p0 >> 32) ^ c.w ^ k.y, static_cast<uint32_t>(p0));
  }
  return c;
}
// key = (lo32, hi32) of the 64-bit key; counter = (lo32, hi32) of the 64-bit counter, then the block index, then 0
__device__ inline uint4 philox_draw(uint64_t key, uint64_t ctr, uint32_t block) {
  return philox4x32_10(make_uint4(static_cast<uint32_t>(ctr), static_cast<uint32_t>(ctr >> 32), block, 0u),
                       make_uint2(static_cast<uint32_t>(key), static_cast<uint32_t>(key >> 32)));
}

// chain.hip: every body sorts its own list ent[ptr[b] .. ptr[b + 1]) ascending (the fill order of an incidence built with
// atomics depends on arrival)
void sort_incidence_lists(size_t n, const int32_t* ptr, int32_t* ent, hipStream_t s);

}  // namespace mhip
