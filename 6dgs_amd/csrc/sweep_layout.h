// sweep_layout.h -- lane / register arithmetic of the select sweep on 16x16x32 MFMAs (k_logits_f16x<.., kOutUB, .., kMfma16>, score.hip), usable
// from device AND host code: the CPU test-suite walks every (lane, register) through these very functions (libsixdgs_hostcheck.so,
// tests/test_sweep_layout.py), so the accumulator map, the butterfly and the store map cannot drift apart unnoticed on a machine without a GPU.
//
// A wave owns 64 token rows x 128 rays of the 256 x 256 tile: 4 token blocks tb x 8 ray blocks rb of 16 x 16, C^T = K Q^T (rows = rays,
// columns = tokens), 4 accumulator registers per block.
#pragma once
#include <hip/hip_runtime.h>

namespace sdg {
namespace sw {

#define SDG_SW __host__ __device__ __forceinline__ constexpr

constexpr int kTokBlocks = 4, kRayBlocks = 8, kBlockBytes = 16 * 128;   // a 16-row block of the LDS image [256 rows][128 B] is 2048 B further on

// operand fragment of lane l: row l & 15 of its 16-row block, 16-byte chunk plane * 4 + (l >> 4) of the row's 128-byte slab (k = 8 (l >> 4) + 0..7)
SDG_SW int frag_row(int lane) { return lane & 15; }
SDG_SW int frag_chunk(int lane, int plane) { return plane * 4 + (lane >> 4); }
// byte offset inside one stage of the image: the eight chunks of a row are XOR-swizzled with (row >> 1) & 7 (on the source side of the DMA)
SDG_SW unsigned frag_offset(int row0, int lane, int plane) {
  const int row = row0 + frag_row(lane);
  return (unsigned)(row * 128 + ((frag_chunk(lane, plane) ^ ((row >> 1) & 7)) << 4));
}

// 16x16 C/D: column = lane & 15 (the token of block tb), row = 4 (lane >> 4) + reg (the ray of block rb); both relative to the wave's corner
SDG_SW int acc_token(int lane, int tb) { return 16 * tb + (lane & 15); }
SDG_SW int acc_ray(int lane, int rb, int reg) { return 16 * rb + 4 * (lane >> 4) + reg; }

// The per-ray sum over the wave's 64 tokens: a lane first adds its 4 token blocks, which leaves 32 values v[i], i = 4 rb + reg, then a halving
// butterfly over the 16 lanes that share lane >> 4.  Step s = 0..3 pairs lane with lane ^ (1 << s) and splits on bit s of i: of v[i] and
// v[i ^ (1 << s)] a lane keeps the one whose bit s equals its own lane bit s, receives the partner's other one and adds.  What is left after
// the four steps is bit 4 of i: two values x = 0, 1 per lane.
constexpr int kBflySteps = 4;
SDG_SW int bfly_partner(int lane, int step) { return lane ^ (1 << step); }
SDG_SW int bfly_keeps(int lane, int step, int i) { return ((i >> step) & 1) == ((lane >> step) & 1); }
// ray (relative to the wave's 128) of the lane's output x: i = 16 x + (lane & 15), rb = i >> 2, reg = i & 3; the 64 lanes of one store
// instruction cover 64 consecutive rays
SDG_SW int out_index(int lane, int x) { return 16 * x + (lane & 15); }
SDG_SW int out_ray(int lane, int x) { return acc_ray(lane, out_index(lane, x) >> 2, out_index(lane, x) & 3); }

// the per-token sums over the rays: the 4 lane groups lane >> 4 hold partial sums of the same token; lanes with bit 4 clear take the partner's
// (lane ^ 16) and write row part_row of the merge buffer [2 wn + (lane >> 5)][256 tokens]
SDG_SW bool part_writes(int lane) { return (lane & 16) == 0; }
SDG_SW int part_row(int wn, int lane) { return 2 * wn + (lane >> 5); }

#undef SDG_SW
}  // namespace sw
}  // namespace sdg
