// Counter-based random numbers for the train patch pipeline: the splitmix64 finaliser pnp.hip uses (restated here;
// pnp.hip keeps its own copy and its bits), keyed by (seed, sample id, stream, counter).  A draw never depends on the
// batch an object travels in or on its position there.
//   hash    h = mix(mix(mix(mix(seed) ^ sample_id) ^ stream) ^ counter)
//   uniform u = ((h >> 40) + 0.5) 2^-24 in fp64: 25 significant bits, exact, inside (0, 1).  Rounded to fp32 where a
//           kernel works in fp32 (the largest value then rounds to 1.0f; 0 is never reached, so ln u stays finite).
//   normal  Box-Muller from ONE hash: u1 from bits 63..40, u2 from bits 39..16, z = sqrt(-2 ln u1) cos(2 pi u2).
#pragma once
#include <stdint.h>

#define SCF_RNG_JITTER 1      // counter = try * 8 + i, i = 0..2 the angles, 3..5 the translation noise
#define SCF_RNG_CROP 2        // counter 0: Crop's size ratio
#define SCF_RNG_HSV 3         // counter 0..2: the h, s, v gains
#define SCF_RNG_SIGMA 4       // counter 0: RandomNoise's sigma
#define SCF_RNG_NOISE 5       // counter = (y pw + x) 3 + c in patch coordinates: the pixel's normal draw
#define SCF_RNG_SMOOTH 6      // counter 0: RandomSmooth's kernel size
#define SCF_RNG_GATE_HSV 7    // counter 0: the three p gates
#define SCF_RNG_GATE_NOISE 8
#define SCF_RNG_GATE_SMOOTH 9

__host__ __device__ __forceinline__ uint64_t scf_rng_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t scf_rng_hash(uint64_t seed, uint64_t sample_id, uint64_t stream, uint64_t counter) {
  return scf_rng_mix(scf_rng_mix(scf_rng_mix(scf_rng_mix(seed) ^ sample_id) ^ stream) ^ counter);
}
__host__ __device__ __forceinline__ double scf_rng_u1(uint64_t h) { return ((double)(h >> 40) + 0.5) * 0x1p-24; }
__host__ __device__ __forceinline__ double scf_rng_u2(uint64_t h) { return ((double)((h >> 16) & 0xFFFFFFull) + 0.5) * 0x1p-24; }
__host__ __device__ __forceinline__ double scf_rng_uniform(uint64_t seed, uint64_t sample_id, uint64_t stream, uint64_t counter) {
  return scf_rng_u1(scf_rng_hash(seed, sample_id, stream, counter));
}
