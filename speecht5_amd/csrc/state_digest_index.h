// Arithmetic of csrc/state_digest.hip (st5_state_digest: one 64-bit digest per segment of a set of device segments -- the checkpoint
// of an update, speecht5_amd/checkpoint.py), as inline functions that compile for the device AND for the host:
// tests/test_checkpoint_cpu.py builds this header with the host compiler and compares, for sets of segment sizes and start offsets,
// the digests it yields against the numpy restatement of the definition (tests/state_digest_reference.py).
//
// Definition (all arithmetic mod 2^64), for a segment of n bytes:
//   w_i    the little-endian 8-byte words of the segment, i = 0 .. ceil(n / 8) - 1, the last one zero-padded
//   digest = h( (sum over i of h(w_i + (i + 1) * 0x9E3779B97F4A7C15)) + n )         h = the splitmix64 finaliser
// The outer sum wraps around, so every reduction order gives the same bits (the kernel adds partial sums with integer atomics); the
// position term makes swapped words visible, n makes trailing zero bytes visible.  h is a bijection of the 64-bit words, so two
// segments that differ in ONE word always differ in the digest.
//
// The chunking is the batch load's (batch_load_index.h): 256-byte chunks spread over the grid, a chunk finds its segment by bisection
// over the chunk prefix, 16 lanes share a chunk and read 16 bytes = two words each.  Nothing here writes memory; sd_lane_sum reads
// the bytes [begin, end) of the segment it is given and nothing else.
#pragma once
#include <stdint.h>
#include "batch_load_index.h"

constexpr uint64_t SD_GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr int SD_MAX_BLOCKS = 2048;       // grid cap of the accumulate kernel: it walks the chunks with a grid stride

// the splitmix64 finaliser
BL_HD uint64_t sd_mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// the summand of word number i (counted from 0 inside its segment)
BL_HD uint64_t sd_term(uint64_t w, uint64_t i) { return sd_mix(w + (i + 1) * SD_GOLDEN); }

// a segment's digest from the wrapped sum of its summands
BL_HD uint64_t sd_finish(uint64_t sum, uint64_t n_bytes) { return sd_mix(sum + n_bytes); }

// the lane may take its 16 bytes as one 128-bit load: a whole lane's worth, the segment's base 16-byte aligned (begin is a multiple of 16)
BL_HD bool sd_vector_ok(uint64_t base, long long begin, long long end) { return end - begin == BL_LANE_BYTES && (base & 15u) == 0; }

// the two words of a full lane, read as such (little-endian host and device), their summands added
BL_HD uint64_t sd_pair_sum(uint64_t w0, uint64_t w1, long long begin) {
  const uint64_t i = (uint64_t)begin / 8;
  return sd_term(w0, i) + sd_term(w1, i + 1);
}

// the summands of the words that the bytes [begin, end) of a segment form, byte by byte: begin is a multiple of 16 (bl_lane_range), so
// words never straddle two lanes; end - begin <= 16; a last word short of 8 bytes is zero-padded; an empty range has no word
// (P: a pointer to bytes -- on the device one into the global address space, so that the reads are global and not flat loads)
template <typename P>
BL_HD uint64_t sd_lane_sum(P seg, long long begin, long long end) {
  uint64_t sum = 0;
  for (long long w = begin; w < end; w += 8) {
    uint64_t word = 0;
    const long long stop = w + 8 < end ? w + 8 : end;
    for (long long k = w; k < stop; ++k) word |= (uint64_t)seg[k] << (8 * (k - w));
    sum += sd_term(word, (uint64_t)w / 8);
  }
  return sum;
}

// workgroups of the accumulate kernel for `chunks` chunks
BL_HD long long sd_blocks(long long chunks) { return bl_blocks(chunks, SD_MAX_BLOCKS); }

// iterations of the grid-stride loop: the same for every thread, so the wave-wide steps inside it run under uniform control flow
BL_HD long long sd_iterations(long long chunks, long long blocks) {
  const long long per = (long long)(BL_THREADS / BL_LANES) * blocks;
  return per <= 0 ? 0 : (chunks + per - 1) / per;
}
