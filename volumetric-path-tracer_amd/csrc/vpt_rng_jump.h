// vpt_rng_jump.h — make_state's per-pixel PCG32 seeds without the sequential master stream (include/vpt.h: vpt_state_init_device).
// Compiled by the state-initialisation kernel (csrc/vpt_frame_stages.hip) and by the host library (make_state_jump): integers only, so
// both give the bits of make_state (yocto_pathtrace.cpp:975-978, yocto_sampling.h:184-205).
// PCG32's state update is the LCG  s' = A s + inc  (mod 2^64), so n steps are  s -> A^n s + inc (A^n - 1) / (A - 1):  the pair
// (A^n, c_n) comes from square-and-multiply over the bits of n (Brown, "Random number generation with arbitrary strides", 1994).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VPT_HD __host__ __device__ inline
#else
#define VPT_HD inline
#endif

struct vpt_pcg32 {
  uint64_t state, inc;
};
struct vpt_lcg_jump {   // n steps of the LCG at once: s -> mul * s + add
  uint64_t mul, add;
};

#define VPT_PCG32_MULT 6364136223846793005ULL
#define VPT_STATE_MASTER_SEED 1301081ULL    // make_rng(1301081): the master stream, default sequence 1
#define VPT_STATE_PIXEL_SEED 961748941ULL   // make_rng(961748941, seq) of every pixel

VPT_HD uint32_t vpt_pcg32_output(uint64_t old) {   // what _advance_rng returns for the state it found
  uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u), rot = (uint32_t)(old >> 59u);
  return (xs >> rot) | (xs << ((~rot + 1u) & 31));
}
VPT_HD vpt_pcg32 vpt_pcg32_make(uint64_t seed, uint64_t seq) {   // make_rng, yocto_sampling.h:184-190
  vpt_pcg32 r = {0, (seq << 1u) | 1u};
  r.state = r.state * VPT_PCG32_MULT + r.inc;
  r.state += seed;
  r.state = r.state * VPT_PCG32_MULT + r.inc;
  return r;
}
VPT_HD vpt_lcg_jump vpt_pcg32_jump(uint64_t inc, uint64_t n) {
  vpt_lcg_jump acc = {1, 0};
  uint64_t     mul = VPT_PCG32_MULT, add = inc;
  for (; n > 0; n >>= 1) {
    if (n & 1) acc.mul = acc.mul * mul, acc.add = acc.add * mul + add;
    add = (mul + 1) * add, mul = mul * mul;
  }
  return acc;
}
// the seed of a pixel from the master stream's state in front of its draw: rand1i(master, 1 << 31) / 2 + 1 names its sequence
VPT_HD vpt_pcg32 vpt_state_pixel_rng(uint64_t master_state) {
  const uint32_t r   = vpt_pcg32_output(master_state);
  const int      seq = (int)(r % 2147483648u) / 2 + 1;
  return vpt_pcg32_make(VPT_STATE_PIXEL_SEED, (uint64_t)seq);
}
// the rng of the pixel with row-major index idx, by one full jump
VPT_HD vpt_pcg32 vpt_state_pixel_rng_at(uint64_t idx) {
  const vpt_pcg32    master = vpt_pcg32_make(VPT_STATE_MASTER_SEED, 1);
  const vpt_lcg_jump j      = vpt_pcg32_jump(master.inc, idx);
  return vpt_state_pixel_rng(j.mul * master.state + j.add);
}
